"""The buffer contract of include/egt_amd.h for egt_pair_block_fwd / egt_pair_block_bwd, through the harness of
tests/memcontract.py: every tensor of the two calls in a guarded arena of exactly its byte count; outputs, `saved` and the
workspace prefilled with 0x00 and with 0xFF (`saved` is carried from the forward to the backward, which completes parts of it;
the workspace is scratch: poisoned again before the backward); the fourteen parameters and the fourteen gradient sinks shifted to
4-byte alignment ("sinks" / "all" / "mixed"); d_e aliasing d_e_out.  Run Z is held to the Python wrapper's result bit for bit
(tests/test_pair_block_gpu.py ties that result to the fp64 oracle)."""
import ctypes as C

import pytest
import torch

import memcontract as M
from memcontract import Buf, Case, IN, OUT, CARRIED, SCRATCH, PARAM, SINK

pytestmark = pytest.mark.gpu
SHAPES = [(1, 37, 29), (2, 48, 40)]          # (B, N, real nodes of the last graph)


def pair_block_case(lib, B, N, real):
    from egt_amd import _lib as L
    from oracle import egt_oracle as O
    d, De, H = 64, 32, 8
    g = M._gen(f"pair_block{B}.{N}")
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    km = torch.ones(B, N, dtype=torch.uint8)
    km[B - 1, real:] = 0
    inp = dict(h=r(B, N, d * H), e=r(B, N, N, De) * 1.3 + 0.2, key_mask=km, d_h_out=r(B, N, d * H), d_e_out=r(B, N, N, De))
    allp = O.init_block_params(d * H, De, H, dtype=torch.float32, generator=g, randomize_norm=True)
    params = {f: allp[k] for f, k in zip(L.BLOCK_PARAM_FIELDS, M.BLOCK_ORACLE_NAMES)}
    desc = L.BlockDesc(B=B, N=N, H=H, d=d, De=De, dtype=L.EGT_F32, flags=L.BF_GATE | L.BF_CLIP | L.BF_TRAINING, clip_lo=-5.0, clip_hi=5.0,
                       random_mask_prob=M.RAND_P, ln_eps=1e-3, reserved=0, seed=M.SEED, seed_device=None)
    p = C.byref(desc)
    bufs = [Buf(k, IN, t, graphs=B) for k, t in inp.items()]
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]
    bufs += [Buf("h_out", OUT, dtype=torch.float32, shape=inp["h"].shape, graphs=B),
             Buf("e_out", OUT, dtype=torch.float32, shape=inp["e"].shape, graphs=B),
             Buf("d_h", OUT, dtype=torch.float32, shape=inp["h"].shape, graphs=B),
             Buf("d_e", OUT, dtype=torch.float32, shape=inp["e"].shape, graphs=B),
             Buf("saved", CARRIED, nbytes=lib.egt_pair_block_saved_bytes(p), graphs=B),
             Buf("ws", SCRATCH, nbytes=lib.egt_pair_block_workspace_bytes(p), graphs=B)]

    def fwd(v):
        return lib.egt_pair_block_fwd(p, C.byref(M._struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, "p.")), M._ptr(v, "h"), M._ptr(v, "e"),
                                      M._ptr(v, "key_mask"), M._ptr(v, "h_out"), M._ptr(v, "e_out"), M._ptr(v, "saved"), M._ptr(v, "ws"),
                                      M._stream())

    def bwd(v):
        return lib.egt_pair_block_bwd(p, C.byref(M._struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, "p.")), M._ptr(v, "h"), M._ptr(v, "e"),
                                      M._ptr(v, "key_mask"), M._ptr(v, "saved"), M._ptr(v, "d_h_out"), M._ptr(v, "d_e_out"),
                                      M._ptr(v, "d_h"), M._ptr(v, "d_e"),
                                      C.byref(M._struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, "g.")), M._ptr(v, "ws"), M._stream())

    def wrapper(dev):
        from egt_amd.pair import _PairBlock
        wd = L.BlockDesc.from_buffer_copy(desc)
        h, e = inp["h"].to(dev).requires_grad_(), inp["e"].to(dev).requires_grad_()
        ps = [t.to(dev).requires_grad_() for t in params.values()]
        h_out, e_out = _PairBlock.apply(h, e, km.to(dev), wd, *ps)
        torch.autograd.backward([h_out, e_out], [inp["d_h_out"].to(dev), inp["d_e_out"].to(dev)])
        out = {"h_out": h_out.detach(), "e_out": e_out.detach(), "d_h": h.grad, "d_e": e.grad}
        out.update({"g." + f: t.grad for f, t in zip(params, ps)})
        return out
    return Case(f"pair_block_b{B}_n{N}", bufs, [fwd, bwd], [{"d_e": "d_e_out"}], desc=desc, wrapper=wrapper,
                supported=lambda: lib.egt_pair_block_supported(p))


@pytest.mark.parametrize("B,N,real", SHAPES)
def test_pair_block_contract(B, N, real, gpu, egt_lib):
    from egt_amd import _lib as L
    case = pair_block_case(egt_lib, B, N, real)
    assert case.claims["supported"]() == 1
    by = {b.name: b for b in case.bufs}
    assert by["saved"].role == CARRIED and by["saved"].nbytes > 0 and by["ws"].role == SCRATCH and by["ws"].nbytes > 0
    tagged = M.tagged(case)
    assert len(tagged) == 28, "fourteen parameters and fourteen sinks"
    for which in M.U_RUNS:
        assert len(M.shifts(case, which)) >= 14, which
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    for name, ref in case.claims["wrapper"](gpu).items():
        got = z[name]
        assert ref.shape == got.shape and ref.dtype == got.dtype, name
        assert torch.equal(got.view(torch.int32), ref.contiguous().view(torch.int32)), f"{name}: differs from the Python wrapper's result"
