"""The buffer contract of include/egt_amd.h for egt_graph_head_fwd / egt_graph_head_bwd, through the harness of
tests/memcontract.py: every tensor of the two calls in a guarded arena of exactly its byte count; outputs and the workspace
prefilled with 0x00 and with 0xFF (the workspace is scratch: poisoned again before the backward); parameters and gradient
sinks shifted to 4-byte alignment ("sinks" / "all" / "mixed"); NULL gamma / beta without EGT_GH_LAYERNORM.  Run Z is held to the
Python wrapper's result bit for bit (tests/test_graph_head_gpu.py ties that result to the fp64 oracle)."""
import ctypes as C

import pytest
import torch

import graph_head_ref as GR
import memcontract as M
from memcontract import Buf, Case, IN, OUT, SCRATCH, PARAM, SINK

pytestmark = pytest.mark.gpu
CASE_IDS = ("w64_mae_n19", "w48_mae_n37", "w64_xent_n19", "w64_mae_b70", "w64_xent_nv2", "w48_xent_nv4", "w64_mae_relu_noln")


def _lib():
    from egt_amd import build, _lib as L
    build.build()
    return L.load()


def graph_head_case(lib, cid):
    from egt_amd import _lib as L
    from egt_amd.graph_head import graph_head_desc
    c = GR.make_case(cid)
    B, N, nv, W, Cc = c["B"], c["N"], c["nv"], c["W"], c["C"]
    desc = graph_head_desc(B, N, W, c["M0"], c["M1"], Cc, nv, c["loss"], c["act"], c["ln"])
    p = C.byref(desc)
    target = c["target"] if c["loss"] == "mae" else c["target"].to(torch.int32)
    inp = dict(h=c["h"], target=target, mask=c["mask"].to(torch.uint8), d_loss=torch.tensor([GR.S_UP]))
    bufs = [Buf(k, IN, t, graphs=B) for k, t in inp.items()]
    params = {f: t for f, t in zip(L.NODE_HEAD_PARAM_FIELDS, c["params"]) if t is not None}     # gamma / beta absent: NULL
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]
    bufs += [Buf("stats", OUT, dtype=torch.float32, shape=(3,)), Buf("pred", OUT, dtype=torch.float32, shape=(B, Cc), graphs=B),
             Buf("d_h", OUT, dtype=torch.float32, shape=(B, nv + N, W), graphs=B),
             Buf("ws", SCRATCH, nbytes=lib.egt_graph_head_workspace_bytes(p), graphs=B)]

    def fwd(v):
        return lib.egt_graph_head_fwd(p, C.byref(M._struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, v, "p.")), M._ptr(v, "h"),
                                      M._ptr(v, "target"), M._ptr(v, "mask"), M._ptr(v, "stats"), M._ptr(v, "pred"), M._ptr(v, "ws"),
                                      M._stream())

    def bwd(v):
        return lib.egt_graph_head_bwd(p, C.byref(M._struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, v, "p.")), M._ptr(v, "h"),
                                      M._ptr(v, "target"), M._ptr(v, "mask"), M._ptr(v, "d_loss"), M._ptr(v, "d_h"),
                                      C.byref(M._struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, v, "g.")), M._ptr(v, "ws"),
                                      M._stream())

    def wrapper(dev):
        from egt_amd.graph_head import graph_head_loss
        got, _ = GR.run(graph_head_loss, c, dev)
        res = {"stats": got["stats"], "pred": got["pred"], "d_h": got["d_h"]}
        res.update({"g." + f: g for f, g in zip(params, got["grads"])})
        return res
    return Case(f"graph_head_{cid}", bufs, [fwd, bwd], desc=desc, wrapper=wrapper, supported=lambda: lib.egt_graph_head_supported(p))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_graph_head_contract(cid, gpu, egt_lib):
    from egt_amd import _lib as L
    case = graph_head_case(egt_lib, cid)
    assert case.claims["supported"]() == 1
    ws = [b for b in case.bufs if b.name == "ws"][0]
    assert ws.role == SCRATCH and ws.nbytes > 0
    tagged = M.tagged(case)
    assert len(tagged) == (16 if GR.CASES[cid][9] else 12), "eight (six without LayerNorm) parameters and as many sinks"
    for which in M.U_RUNS:
        assert M.shifts(case, which), which
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    for name, ref in case.claims["wrapper"](gpu).items():
        got = z[name]
        assert ref.shape == got.shape and ref.dtype == got.dtype, name
        assert torch.equal(got.view(torch.int32), ref.contiguous().view(torch.int32)), f"{name}: differs from the Python wrapper's result"
