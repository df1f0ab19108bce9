"""GPU parity of the MFMA inner op's bf16-product mode (EGT_ATTN_MM_BF16, AttnConfig(matmul="bf16"); egt_attn_bf16.hip): forward +
backward through egt_attention against the fp64 oracle.

Per case: H_hat at the suite's FWD and dG at its BWD tolerance against the oracle fed the ROUNDED operands (these two carry no
bf16 error under the contract); V_att, dQKV and dE at ATTN_BF16_TOL against the same oracle (tests/attn_bf16_ref.py: half of
BF16_TOL elementwise, three times the emulated L2 error; tests/test_attn_bf16_cpu.py shows the contract alone uses at most half
of it); every tensor at BF16_TOL against the PLAIN oracle.

EGT_ATTN_BF16_MARGINS=<path>: the worst error / tolerance of every parity case is written there (JSON) when the module ends
(profiles/attn_bf16_margins.json is such a dump)."""
import ctypes as C
import functools
import json
import os

import pytest
import torch

import attn_bf16_ref as R
import cases as CS
from util import assert_close, margin, FWD, BWD

pytestmark = pytest.mark.gpu
MARGINS = {}
KERNELS = ("k_attn_bf16_pack", "k_attn_bf16_fwd", "k_attn_bf16_bwd_kv", "k_attn_bf16_bwd_q")
strip = lambda t: {k: v for k, v in t.items() if k in ("rtol", "arel")}


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    path = os.environ.get("EGT_ATTN_BF16_MARGINS")
    if path and MARGINS:
        json.dump(MARGINS, open(path, "w"), indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def references(name):
    """(inp, attrs, d, plain oracle, oracle fed the rounded operands) of a table case: computed once, shared, left unchanged"""
    inp, attrs = R.make_case(name)
    d = R.CASES[name][2]
    return inp, attrs, d, CS.attn_oracle(inp, attrs), R.oracle_rounded(inp, attrs, d)


def run_hip(inp, attrs, dev, matmul="bf16", p=None, seed=0, inject=True):
    """forward + backward through egt_attention; p: random_mask_prob (the mask bytes are injected when the case has them and
    `inject`, drawn in the kernel otherwise)"""
    from egt_amd import egt_attention, AttnConfig
    cu = lambda t: None if t is None else t.to(dev)
    q = cu(inp["QKV"]).requires_grad_(); e_ = cu(inp["E"]).requires_grad_()
    g_ = cu(inp["G"]).requires_grad_() if inp["G"] is not None else None
    rm = inp["rand_mask"] if inject else None
    if p is None:
        p = 0.5 if rm is not None else 0.0
    cfg = AttnConfig(num_heads=R.H, clip_logits_value=attrs["clip_logits_value"], random_mask_prob=p, training=p > 0.0, seed=seed,
                     need_a_tild=False, use_mfma=True, matmul=matmul)
    V, Hh, _ = egt_attention(q, e_, g_, cu(inp["M"]), cu(inp["mask"]), cfg=cfg, rand_mask=cu(rm))
    torch.autograd.backward([V, Hh], [cu(inp["dV"]), cu(inp["dH"])])
    return dict(V_att=V.detach(), H_hat=Hh.detach(), dQKV=q.grad, dE=e_.grad, dG=None if g_ is None else g_.grad)


def compare(tag, out, plain, rounded):
    m = {}
    for k, tol in (("H_hat", FWD), ("dG", BWD), ("V_att", R.ATTN_BF16_TOL), ("dQKV", R.ATTN_BF16_TOL), ("dE", R.ATTN_BF16_TOL)):
        if rounded[k] is not None:
            m[k] = margin(out[k], rounded[k], **strip(tol))
            m[k + " vs plain / BF16_TOL"] = margin(out[k], plain[k], **strip(R.BF16_TOL))
    for k in ("V_att", "dQKV", "dE"):
        m[k + " L2 / ATTN_BF16_TOL"] = float((out[k].double().cpu() - rounded[k]).norm() / rounded[k].norm()) / R.ATTN_BF16_TOL["l2"]
    MARGINS[tag] = m
    print(f"[attn_bf16 margins] {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()))
    assert_close(out["H_hat"], rounded["H_hat"], name="H_hat vs rounded-operand oracle", **FWD)
    if rounded["dG"] is not None:
        assert_close(out["dG"], rounded["dG"], name="dG vs rounded-operand oracle", **BWD)
    for k in ("V_att", "dQKV", "dE"):
        assert_close(out[k], rounded[k], name=k + " vs rounded-operand oracle", **R.ATTN_BF16_TOL)
    for k in ("V_att", "H_hat", "dQKV", "dE", "dG"):
        if plain[k] is not None:
            assert_close(out[k], plain[k], name=k + " vs plain oracle", **R.BF16_TOL)


@pytest.mark.parametrize("name", list(R.CASES))
def test_attn_bf16_vs_oracle(name, gpu, egt_lib):
    inp, attrs, d, plain, rounded = references(name)
    compare(name, run_hip(inp, attrs, gpu), plain, rounded)


@pytest.mark.parametrize("name", list(R.RNG_CASES))
def test_attn_bf16_in_kernel_random_mask(name, gpu, egt_lib):
    """the straight-line instances with the in-kernel mask stream; the oracle is fed mask_sample's bytes"""
    from egt_amd import mask_sample
    B, N, d = R.RNG_CASES[name]
    rm = mask_sample(0, R.RNG_SEED, R.RNG_P, B, N, R.H, gpu).cpu().bool()
    inp, attrs = R.make_rng_case(name, rm)
    out = run_hip(inp, attrs, gpu, p=R.RNG_P, seed=R.RNG_SEED, inject=False)
    compare(name, out, CS.attn_oracle(inp, attrs), R.oracle_rounded(inp, attrs, d))


def _counts(lib):
    out = {}
    for nm in KERNELS + ("k_attn_pack", "k_attn_mfma_fwd", "k_attn_mfma_bwd_kv", "k_attn_mfma_bwd_q"):
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(nm.encode(), C.byref(cnt), C.byref(ms))
        out[nm] = cnt.value
    return out


@pytest.mark.parametrize("name", ["n48_d64", "n37_d16", "n21_d32_ungated"])
def test_the_bf16_kernels_ran_and_are_deterministic(name, gpu, egt_lib):
    """the launch profiler counts the four bf16 kernels and none of the fp32 ones; V_att differs from the fp32 mode's in its bits
    (and by no more than BF16_TOL); a second run is bit-equal"""
    inp, attrs, d, plain, _ = references(name)
    egt_lib.egt_prof_filter(b""); egt_lib.egt_prof_enable(2)
    try:
        a = run_hip(inp, attrs, gpu)
        torch.cuda.synchronize()
    finally:
        egt_lib.egt_prof_enable(0)
    n = _counts(egt_lib)
    assert all(n[k] == 1 for k in KERNELS if k != "k_attn_bf16_pack") and n["k_attn_bf16_pack"] == 2, n
    assert all(n[k] == 0 for k in n if k not in KERNELS), n
    f32 = run_hip(inp, attrs, gpu, matmul="f32")
    assert not torch.equal(a["V_att"], f32["V_att"]) and not torch.equal(a["dQKV"], f32["dQKV"])
    assert_close(a["V_att"], f32["V_att"], name="V_att bf16 vs f32 mode", **R.BF16_TOL)
    assert_close(f32["V_att"], plain["V_att"], name="V_att f32 mode", **FWD)       # the default stayed exact
    b = run_hip(inp, attrs, gpu)
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["n48_d64", "n37_d16", "n21_d32"])
def test_attn_bf16_workspace_modes(name, gpu, egt_lib, monkeypatch):
    """shared-workspace backward, a second backward under retain_graph, the re-packing backward (EGT_ATTN_WS_SHARED=0) and a
    torch.no_grad() forward on the forward-only workspace: all bit-equal"""
    from egt_amd import egt_attention, AttnConfig, _lib as L
    inp, attrs, d, _, _ = references(name)
    cu = lambda t: None if t is None else t.to(gpu)
    cfg = AttnConfig(num_heads=R.H, need_a_tild=False, use_mfma=True, matmul="bf16")
    leaves = lambda: [cu(inp[k]).clone().requires_grad_() for k in ("QKV", "E", "G")]
    q, e_, g_ = leaves()
    V, Hh, _ = egt_attention(q, e_, g_, None, cu(inp["mask"]), cfg=cfg)
    assert V.grad_fn.saved_tensors[-1] is not None, "a forward that will be differentiated takes the shared workspace"
    assert V.grad_fn.desc.reserved == L.ATTN_WS_SHARED | L.ATTN_MM_BF16
    torch.autograd.backward([V, Hh], [cu(inp["dV"]), cu(inp["dH"])], retain_graph=True)
    first = [t.grad.clone() for t in (q, e_, g_)]
    q.grad = e_.grad = g_.grad = None
    torch.autograd.backward([V, Hh], [cu(inp["dV"]), cu(inp["dH"])])
    for a, b, n in zip(first, (q.grad, e_.grad, g_.grad), ("dQKV", "dE", "dG")):
        assert torch.equal(a, b), n + " (second backward)"
    monkeypatch.setenv("EGT_ATTN_WS_SHARED", "0")
    q2, e2, g2 = leaves()
    Vn, Hn, _ = egt_attention(q2, e2, g2, None, cu(inp["mask"]), cfg=cfg)
    assert Vn.grad_fn.saved_tensors[-1] is None and Vn.grad_fn.desc.reserved == L.ATTN_MM_BF16
    torch.autograd.backward([Vn, Hn], [cu(inp["dV"]), cu(inp["dH"])])
    for a, b, n in zip(first, (q2.grad, e2.grad, g2.grad), ("dQKV", "dE", "dG")):
        assert torch.equal(a, b), n + " (re-packing backward)"
    monkeypatch.delenv("EGT_ATTN_WS_SHARED")
    with torch.no_grad():
        V2, Hh2, _ = egt_attention(cu(inp["QKV"]), cu(inp["E"]), cu(inp["G"]), None, cu(inp["mask"]), cfg=cfg)
    assert torch.equal(V2, V) and torch.equal(Hh2, Hh) and torch.equal(Vn, V)


def test_refused_where_the_mfma_path_is_not_taken(gpu, egt_lib):
    """matmul='bf16' on a call the MFMA inner op does not take is a ValueError, never a silent fp32 run"""
    from egt_amd import egt_attention, AttnConfig
    mk = lambda d, N=8: (torch.randn(1, N, 3 * d * R.H, device=gpu), torch.randn(1, N, N, R.H, device=gpu), torch.randn(1, N, N, R.H, device=gpu))
    for d, kw in ((8, {}), (16, dict(scale_degree=True)), (16, dict(attn_dropout=0.1, training=True)), (16, dict(need_a_tild=True)),
                  (16, dict(use_mfma=False)), (24, {})):
        q, e_, g_ = mk(d)
        with pytest.raises(ValueError, match="bf16"):
            egt_attention(q, e_, g_, cfg=AttnConfig(matmul="bf16", **dict(dict(need_a_tild=False), **kw)))
    q, e_, g_ = mk(16)
    with pytest.raises(ValueError, match="bf16"):       # injected dropout samples send a call to the general kernel as well
        egt_attention(q, e_, g_, cfg=AttnConfig(matmul="bf16", need_a_tild=False), drop_keep=torch.ones(1, 8, 8, R.H, dtype=torch.uint8, device=gpu))


def test_c_abi_flags_and_general_backward(gpu, egt_lib):
    """reserved = EGT_ATTN_MM_BF16 | 0x40 is EGT_E_FLAGS; the rowstats layout is the default mode's, so a forward with the bit pairs
    with egt_attn_bwd (the general kernel).  That backward reads the UNROUNDED q / k / v / dV_att: the bf16 noise reaches it only
    through rowstats (max and sum of logits that differ from the exact ones by ~1e-3) and V_att (delta), so its reference is the
    plain oracle, at ATTN_BF16_TOL."""
    from egt_amd import _lib as L
    from egt_amd.functional import AttnConfig, _attn_desc
    inp, attrs, d, plain, _ = references("n21_d32")
    B, N = inp["QKV"].shape[:2]
    cu = lambda t: None if t is None else t.to(gpu).contiguous()
    qkv, E, G, km = cu(inp["QKV"]), cu(inp["E"]), cu(inp["G"]), cu(inp["mask"].to(torch.uint8))
    dV, dH = cu(inp["dV"]), cu(inp["dH"])
    desc = _attn_desc(AttnConfig(need_a_tild=False), B, N, d, True, True, False)
    v_att = torch.empty(B, N, d * R.H, device=gpu); h_hat = torch.empty(B, N, N, R.H, device=gpu)
    rowstats = torch.empty(B, N, R.H, 4, device=gpu)
    desc.reserved = L.ATTN_MM_BF16 | 0x40
    ws = torch.empty(max(16, egt_lib.egt_attn_mfma_workspace_bytes(C.byref(desc))), dtype=torch.uint8, device=gpu)
    fwd = lambda: egt_lib.egt_attn_mfma_fwd(C.byref(desc), L.ptr(qkv), L.ptr(E), L.ptr(G), L.ptr(km), None, None, L.ptr(v_att), L.ptr(h_hat),
                                            L.ptr(rowstats), L.ptr(ws), L.current_stream())
    assert fwd() == L.EGT_E_FLAGS
    desc.reserved = L.ATTN_MM_BF16
    L.check(fwd())
    desc.reserved = 0
    d_qkv, d_E, d_G = torch.empty_like(qkv), torch.empty_like(E), torch.empty_like(G)
    ws2 = torch.empty(max(16, egt_lib.egt_attn_bwd_workspace_bytes(C.byref(desc))), dtype=torch.uint8, device=gpu)
    L.check(egt_lib.egt_attn_bwd(C.byref(desc), L.ptr(qkv), L.ptr(E), L.ptr(G), L.ptr(km), None, None, None, L.ptr(v_att), L.ptr(rowstats),
                                 L.ptr(dV), L.ptr(dH), L.ptr(d_qkv), L.ptr(d_E), L.ptr(d_G), L.ptr(ws2), L.current_stream()))
    torch.cuda.synchronize()
    m = {k: margin(t, plain[k], **strip(R.ATTN_BF16_TOL)) for k, t in (("dQKV", d_qkv), ("dE", d_E), ("dG", d_G))}
    MARGINS["general_backward_after_bf16_forward"] = m
    print("[attn_bf16 margins] general backward after a bf16 forward: " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()))
    for k, t in (("dQKV", d_qkv), ("dE", d_E), ("dG", d_G)):
        assert_close(t, plain[k], name=k + " (egt_attn_bwd after a bf16 forward)", **R.ATTN_BF16_TOL)


def test_block_with_bf16_attention(gpu, egt_lib):
    """EGTBlock(model_width=128, edge_width=32, attn_matmul='bf16') (d = 16) at N = 19: the composed route, the bf16 kernels ran,
    every output and gradient within BF16_TOL of the block oracle"""
    from egt_amd import EGTBlock
    from test_block_gpu import PMAP
    case = dict(B=2, N=19, Dh=128, De=32, nodes=[19, 12])
    inp, params, attrs, _ = CS.make_block_case("residual_zinc500k", case=case)
    ref = CS.block_oracle(inp, params, attrs)
    blk = EGTBlock(model_width=128, edge_width=32, num_heads=8, attn_matmul="bf16").to(gpu)
    with torch.no_grad():
        for k, (mname, a) in PMAP.items():
            getattr(getattr(blk, mname), a).copy_(params[k].to(gpu))
    h = inp["h"].to(gpu).requires_grad_(); e = inp["e"].to(gpu).requires_grad_()
    egt_lib.egt_prof_filter(b""); egt_lib.egt_prof_enable(2)
    try:
        h2, e2 = blk(h, e, inp["mask"].to(gpu))
        torch.autograd.backward([h2, e2], [inp["dh"].to(gpu), inp["de"].to(gpu)])
        torch.cuda.synchronize()
    finally:
        egt_lib.egt_prof_enable(0)
    assert blk.last_path == "composed"
    n = _counts(egt_lib)
    assert all(n[k] > 0 for k in KERNELS) and n["k_attn_mfma_fwd"] == 0, n
    m = {}
    for k, got in (("h_out", h2), ("e_out", e2), ("dh", h.grad), ("de", e.grad)):
        m[k] = margin(got, ref[k], **strip(R.BF16_TOL))
        assert_close(got, ref[k], name=k, **R.BF16_TOL)
    for k, g in ref["dparams"].items():
        mname, a = PMAP[k]
        got = getattr(getattr(blk, mname), a).grad
        m[k] = margin(got, g, **strip(R.BF16_TOL))
        assert_close(got, g, name=k, **R.BF16_TOL)
    MARGINS["block_w128_de32_n19 vs plain / BF16_TOL"] = m
    print("[attn_bf16 margins] block: worst " + max(m, key=m.get) + f" {max(m.values()):.3f}")
