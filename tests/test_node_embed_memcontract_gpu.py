"""The buffer contract of include/egt_amd.h for egt_node_embed_fwd / egt_node_embed_bwd, through the harness of
tests/memcontract.py: every tensor of the two calls in a guarded arena of exactly its byte count; outputs and the workspace
prefilled with 0x00 and with 0xFF (the workspace is scratch: poisoned again before the backward); parameters, gradient sinks
and -- these kernels hold them to element alignment too -- h_out, mask_out and d_h shifted to 4-byte alignment ("sinks" / "all"
/ "mixed"), then every one of them 1, 2 and 3 floats off at once; pointers the geometry does not use are NULL.  Inputs are
held to their snapshot.  Run Z is held to the Python wrapper's result bit for bit (tests/test_node_embed_gpu.py ties that
result to the fp64 oracle)."""
import ctypes as C

import pytest
import torch

import memcontract as M
import node_embed_cases as NC
from memcontract import Buf, Case, IN, OUT, SCRATCH, PARAM, SINK

pytestmark = pytest.mark.gpu
CASE_IDS = ("lookup", "w48_eig", "empty_n65_vn1_svd", "w16_nv2", "w32_nv16", "float5_svd_nv1", "float3", "svd_notransform",
            "eig_transform", "b37_n40_svd_vn1")


def node_embed_case(lib, cid):
    from egt_amd import _lib as L
    from egt_amd.node_embed import node_embed_desc
    c = NC.make(cid)
    B, N, Dh, nv = c["B"], c["N"], c["Dh"], c["nv"]
    kind, sel, T, transform = c["pe"] or (None, 0, 0, False)
    signs = None if c["signs"] is None else c["signs"].reshape(B, -1).contiguous()
    desc = node_embed_desc(B, N, Dh, nv, c.get("R", 0), c.get("F", 0), kind, T, sel, transform, signs is not None, -1.0,
                           0 if signs is None else signs.shape[1])
    p = C.byref(desc)
    bufs = [Buf("features", IN, c["features"], graphs=B), Buf("d_h", IN, c["d_h"], graphs=B, ptr=PARAM)]
    if kind:
        bufs += [Buf("pe", IN, c["pe_t"], graphs=B), Buf("signs", IN, signs, graphs=B)]
    params = {f: t for f, t in c["params"].items() if t is not None}
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]
    bufs += [Buf("h_out", OUT, dtype=torch.float32, shape=(B, nv + N, Dh), graphs=B, ptr=SINK),
             Buf("mask_out", OUT, dtype=torch.uint8, shape=(B, nv + N), graphs=B, ptr=SINK),
             Buf("ws", SCRATCH, nbytes=lib.egt_node_embed_workspace_bytes(p), graphs=B)]

    def fwd(v):
        return lib.egt_node_embed_fwd(p, C.byref(M._struct(L.NodeEmbedParams, L.NODE_EMBED_PARAM_FIELDS, v, "p.")), M._ptr(v, "features"),
                                      M._ptr(v, "pe"), M._ptr(v, "signs"), M._ptr(v, "h_out"), M._ptr(v, "mask_out"), M._stream())

    def bwd(v):
        return lib.egt_node_embed_bwd(p, M._ptr(v, "features"), M._ptr(v, "pe"), M._ptr(v, "signs"), M._ptr(v, "d_h"),
                                      C.byref(M._struct(L.NodeEmbedParams, L.NODE_EMBED_PARAM_FIELDS, v, "g.")), M._ptr(v, "ws"),
                                      M._stream())

    def wrapper(dev):
        from egt_amd.node_embed import node_embed
        a, prm = NC.args(c, torch.float32, dev)
        h, mask = node_embed(*a)
        res = {"h_out": h.detach(), "mask_out": mask.view(torch.uint8)}
        res.update({"g." + f: g for f, g in NC.grads(h, prm, c["d_h"]).items()})
        return res
    return Case(f"node_embed_{cid}", bufs, [fwd, bwd], desc=desc, wrapper=wrapper, supported=lambda: lib.egt_node_embed_supported(p))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_node_embed_contract(cid, gpu, egt_lib):
    from egt_amd import _lib as L
    case = node_embed_case(egt_lib, cid)
    assert case.claims["supported"]() == 1
    ws = [b for b in case.bufs if b.name == "ws"][0]
    assert ws.role == SCRATCH and ws.nbytes > 0
    tagged = M.tagged(case)
    n_params = sum(t is not None for t in NC.make(cid)["params"].values())
    assert len(tagged) == 2 * n_params + 3, "every parameter and its sink, h_out, mask_out and d_h"
    for which in M.U_RUNS:
        assert M.shifts(case, which), which
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    for floats in (1, 2, 3):                     # every output, sink, parameter and d_h off alignment by the same amount
        u = M.run(case, M.POISON, gpu, sync=torch.cuda.synchronize, check_rc=L.check, shift={b.name: 4 * floats for b in tagged})
        M.assert_same_bits(case, z, u, names=("Z", f"U-{floats}f"))
        M.assert_finite(case, u, f"U-{floats}f")
    for name, ref in case.claims["wrapper"](gpu).items():
        got = z[name]
        assert ref.shape == got.shape and ref.dtype == got.dtype, name
        itype = torch.int32 if got.dtype == torch.float32 else torch.uint8
        assert torch.equal(got.view(itype), ref.contiguous().view(itype)), f"{name}: differs from the Python wrapper's result"
