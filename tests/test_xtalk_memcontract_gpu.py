"""The buffer contract of the cross-talk entry points (include/egt_amd.h: egt_xtalk_supported / _workspace_bytes / _fwd / _bwd) in
the guarded arenas of tests/memcontract.py: every tensor of a call in a buffer of exactly the stated byte count between seeded
guards; outputs, gradient sinks and the workspace prefilled with 0x00 (run Z) and 0xFF (run P); parameters and gradient sinks
also 4, 8 or 12 bytes past the 512-byte boundary (runs U).  Asserted by memcontract.check: guards and const inputs untouched,
runs P and U finite, Z == P == U bit for bit -- so every element of e_out, hn, d_e, d_hr, d_hc and the six parameter gradients
is written, and nothing the workspace held before a call (the forward's contents included: it is poisoned again before the
backward) reaches a result.  Run Z is also held to the fp64 restatement (util.FWD / util.BWD)."""
import ctypes as C

import pytest
import torch

import memcontract as M
import xtalk_cases as XC
from util import assert_close, FWD, BWD

pytestmark = pytest.mark.gpu

# (B, N, De, Dh, s_e, s_n, activation): both sides; De = 64 with two workgroups per graph; each side alone (the other side's
# pointers NULL); every edge-FFN hidden channel handed over; De = 64 with four exchange tiles (the backward's second walk over d e')
TABLE = [(2, 19, 16, 64, 4, 16, "elu"), (1, 37, 64, 48, 16, 12, "relu"), (2, 9, 32, 64, 8, 0, "elu"), (2, 21, 32, 64, 0, 32, "relu"),
         (2, 9, 16, 64, 16, 20, "elu"), (1, 21, 64, 64, 16, 64, "elu")]


def _lib():
    from egt_amd import build, _lib as L
    build.build()
    return L.load()


def xtalk_case(lib, B, N, De, Dh, s_e, s_n, act):
    L = M._L()
    g = M._gen(f"xtalk{De}_{s_e}_{s_n}")
    rn = lambda *s: torch.randn(*s, generator=g)
    params = XC.ffn_params(De, 2 * De - 2 * s_e + s_n, g)
    mask = (torch.arange(N)[None, :] < torch.tensor([N - 3 * b for b in range(B)])[:, None]).float()
    inp = dict(e=rn(B, N, N, De) * 1.5 + 0.2, mask=mask, d_e_out=rn(B, N, N, De))
    if s_n:
        inp.update(hr=rn(B, N, s_n), hc=rn(B, N, s_n))
    if s_e:
        inp.update(d_hn=rn(B, N, s_e))
    desc = L.XtalkDesc(B=B, N=N, De=De, Dh=Dh, s_e=s_e, s_n=s_n, dtype=L.EGT_F32, activation=L.ACT_ELU if act == "elu" else L.ACT_RELU,
                       ln_eps=1e-3, flags=0, reserved=0)
    p = C.byref(desc)
    f32 = torch.float32
    bufs = [M.Buf(k, M.IN, t, graphs=B) for k, t in inp.items()]
    bufs += [M.Buf("e_out", M.OUT, dtype=f32, shape=(B, N, N, De), graphs=B), M.Buf("d_e", M.OUT, dtype=f32, shape=(B, N, N, De), graphs=B),
             M.Buf("ws", M.SCRATCH, nbytes=lib.egt_xtalk_workspace_bytes(p))]
    if s_e:
        bufs.append(M.Buf("hn", M.OUT, dtype=f32, shape=(B, N, s_e), graphs=B))
    if s_n:
        bufs += [M.Buf("d_hr", M.OUT, dtype=f32, shape=(B, N, s_n), graphs=B), M.Buf("d_hc", M.OUT, dtype=f32, shape=(B, N, s_n), graphs=B)]
    for f, t in params.items():
        bufs += [M.Buf("p." + f, M.IN, t, ptr=M.PARAM), M.Buf("g." + f, M.OUT, dtype=f32, shape=t.shape, ptr=M.SINK)]
    ptr, st = M._ptr, M._struct

    def fwd(v):
        return lib.egt_xtalk_fwd(p, C.byref(st(L.FfnParams, L.FFN_PARAM_FIELDS, v, "p.")), ptr(v, "e"), ptr(v, "mask"), ptr(v, "hr"),
                                 ptr(v, "hc"), ptr(v, "e_out"), ptr(v, "hn"), ptr(v, "ws"), M._stream())

    def bwd(v):
        return lib.egt_xtalk_bwd(p, C.byref(st(L.FfnParams, L.FFN_PARAM_FIELDS, v, "p.")), ptr(v, "e"), ptr(v, "mask"), ptr(v, "hr"),
                                 ptr(v, "hc"), ptr(v, "d_e_out"), ptr(v, "d_hn"), ptr(v, "d_e"), ptr(v, "d_hr"), ptr(v, "d_hc"),
                                 C.byref(st(L.FfnParams, L.FFN_PARAM_FIELDS, v, "g.")), ptr(v, "ws"), M._stream())

    def oracle():
        d = torch.float64
        e = inp["e"].to(d).requires_grad_()
        hr, hc = (inp[k].to(d).requires_grad_() for k in ("hr", "hc")) if s_n else (None, None)
        pe = {k: t.to(d).requires_grad_() for k, t in params.items()}
        e2, hn = XC.xtalk_edge_ref(e, inp["mask"], hr, hc, pe, s_e, s_n, act)
        leaves = [e] + ([hr, hc] if s_n else []) + [pe[k] for k in XC.FFN_NAMES]
        gr = list(torch.autograd.grad([e2] + ([hn] if s_e else []), leaves,
                                      [inp["d_e_out"].to(d)] + ([inp["d_hn"].to(d)] if s_e else [])))
        out = {"e_out": (e2.detach(), False), "d_e": (gr.pop(0), True)}
        if s_e:
            out["hn"] = (hn.detach(), False)
        if s_n:
            out["d_hr"], out["d_hc"] = (gr.pop(0), True), (gr.pop(0), True)
        out.update({"g." + k: (t, True) for k, t in zip(XC.FFN_NAMES, gr)})
        return out
    return M.Case(f"xtalk_n{N}_de{De}_se{s_e}_sn{s_n}", bufs, [fwd, bwd], desc=desc, oracle=oracle, supported=lambda: lib.egt_xtalk_supported(p))


CASES = [pytest.param(c, id=c.name) for c in (xtalk_case(_lib(), *row) for row in TABLE)]


@pytest.mark.parametrize("case", CASES)
def test_xtalk_contract(case, gpu, egt_lib):
    from egt_amd import _lib as L
    assert case.claims["supported"]() == 1
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    ref = case.claims["oracle"]()
    assert set(ref) == set(z), set(ref) ^ set(z)
    for name, (r, is_grad) in ref.items():
        assert_close(z[name], r, name=f"{case.name}:{name} vs the fp64 restatement", **(BWD if is_grad else FWD))


def test_size_query_is_what_the_calls_use(egt_lib):
    """one size serves both directions and is 0 for a descriptor the library declines"""
    from egt_amd import _lib as L
    for c in CASES:
        d = c.values[0].claims["desc"]
        assert egt_lib.egt_xtalk_workspace_bytes(C.byref(d)) > 0
    bad = L.XtalkDesc(B=2, N=9, De=48, Dh=48, s_e=4, s_n=4, dtype=L.EGT_F32, activation=L.ACT_ELU, ln_eps=1e-3, flags=0, reserved=0)
    assert egt_lib.egt_xtalk_supported(C.byref(bad)) == 0 and egt_lib.egt_xtalk_workspace_bytes(C.byref(bad)) == 0
