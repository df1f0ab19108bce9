"""The large-head block operator on the GPU (egt_pair_block_fwd / egt_pair_block_bwd, egt_amd/csrc/egt_pair_node.hip): the node
side of mha_block on the library's own fp32 MFMA GEMMs around the fused pair operator.  Every row of
tests/pair_block_cases.py against the fp64 oracle, through egt_amd.pair.block_pair(node="library") and through the raw C entry
points (bit-equal); against the torch node side; training mode, clip off, ill-conditioned inputs, launches, hipGraph capture and
direct gradient sinks."""
import copy
import ctypes as C

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import cases as CS
import conditioning as CD
import pair_block_cases as PB
from util import assert_close, FWD, BWD
from test_block_gpu import build_block, PMAP

pytestmark = pytest.mark.gpu

ATTRS = dict(gate_attention=True, edge_activation=None, edge_channel_type="residual")
KERNELS = {"k_pn_stats", "k_pn_qkv", "k_pn_out", "k_pn_dvatt", "k_pn_dln", "k_pn_lnbwd", "k_pn_wgrad", "k_pn_reduce"}


def _block(params, gpu, rand_p=None):
    return build_block(dict(Dh=PB.DH, De=PB.DE, rand_p=rand_p), ATTRS, params, gpu, "auto")


def _grads(blk):
    return {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items()}


def _run(blk, inp, gpu, node, dh=True, de=True):
    """forward + backward through block_pair with the node side forced: (h', e', dh, de, {parameter gradients})"""
    from egt_amd.pair import block_pair
    hg = inp["h"].to(gpu).requires_grad_(); eg = inp["e"].to(gpu).requires_grad_()
    for p in blk.parameters():
        p.grad = None
    h2, e2 = block_pair(blk, hg, eg, inp["mask"].to(gpu), node=node)
    pairs = [(o, u.to(gpu)) for o, u, on in ((h2, inp["dh"], dh), (e2, inp["de"], de)) if on and u is not None]
    torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
    return h2.detach(), e2.detach(), hg.grad, eg.grad, {k: g.clone() for k, g in _grads(blk).items()}


def _raw(lib, inp, params, gpu, desc):
    """the same call through the C ABI alone"""
    from egt_amd import _lib as L
    f = lambda t: t.to(gpu).float().contiguous()
    h, e, dh, de = f(inp["h"]), f(inp["e"]), f(inp["dh"]), f(inp["de"])
    km = inp["mask"].to(gpu).to(torch.uint8).contiguous()
    ps = [f(params[k]) for k in PMAP]                  # PMAP is in egt_block_params order
    assert [m + "_" + a for m, a in PMAP.values()] == list(L.BLOCK_PARAM_FIELDS)
    gs = [torch.full_like(p, float("nan")) for p in ps]
    h2, e2, d_h, d_e = (torch.full_like(t, float("nan")) for t in (h, e, h, e))
    p = C.byref(desc)
    saved = torch.empty(lib.egt_pair_block_saved_bytes(p), dtype=torch.uint8, device=gpu)
    ws = torch.empty(lib.egt_pair_block_workspace_bytes(p), dtype=torch.uint8, device=gpu)
    st = L.current_stream()
    P = L.params_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, ps)
    G = L.params_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, gs)
    L.check(lib.egt_pair_block_fwd(p, C.byref(P), L.ptr(h), L.ptr(e), L.ptr(km), L.ptr(h2), L.ptr(e2), L.ptr(saved), L.ptr(ws), st))
    ws.fill_(255)                                       # scratch: nothing travels through it
    L.check(lib.egt_pair_block_bwd(p, C.byref(P), L.ptr(h), L.ptr(e), L.ptr(km), L.ptr(saved), L.ptr(dh), L.ptr(de), L.ptr(d_h),
                                   L.ptr(d_e), C.byref(G), L.ptr(ws), st))
    torch.cuda.synchronize()
    return h2, e2, d_h, d_e, dict(zip(PMAP, gs))


def _compare(out, ref):
    h2, e2, dh, de, grads = out
    assert_close(h2, ref["h_out"], name="h_out", **FWD)
    assert_close(e2, ref["e_out"], name="e_out", **FWD)
    assert_close(dh, ref["dh"], name="dh", **BWD)
    assert_close(de, ref["de"], name="de", **BWD)
    for k in PMAP:
        assert_close(grads[k], ref["dparams"][k], name=k, **BWD)


def _same(a, b, what):
    for n, u, v in zip(("h_out", "e_out", "dh", "de"), a[:4], b[:4]):
        assert torch.equal(u, v), f"{what}: {n} differs (max |d| = {(u - v).abs().max().item():.3e})"
    for k in PMAP:
        assert torch.equal(a[4][k], b[4][k]), f"{what}: {k} differs (max |d| = {(a[4][k] - b[4][k]).abs().max().item():.3e})"


@pytest.mark.parametrize("i", range(len(PB.TABLE)), ids=PB.IDS)
def test_rows_vs_oracle_wrapper_and_raw(i, gpu, egt_lib):
    B, N, nodes = PB.TABLE[i]
    inp, params = PB.make(B, N, nodes)
    blk = _block(params, gpu).eval()
    out = _run(blk, inp, gpu, "library")
    _compare(out, PB.oracle(i))
    raw = _raw(egt_lib, inp, params, gpu, PB.desc(B, N))
    _same(out, raw, "block_pair(node='library') vs the raw C entry points")


def test_library_equals_torch_node_side_and_is_deterministic(gpu, egt_lib):
    from oracle import egt_oracle as O  # noqa: F401  (the seeds of tests/test_pair_gpu.py's case)
    inp, params = PB.make(2, 64, [64, 50], seed=7)
    blk = _block(params, gpu).eval()
    a = _run(blk, inp, gpu, "library")
    a2 = _run(blk, inp, gpu, "library")
    _same(a, a2, "two runs of the library route")
    b = _run(blk, inp, gpu, "torch")
    for n, u, v in zip(("h_out", "e_out"), a[:2], b[:2]):
        assert_close(u, v, name=n, rtol=1e-4, arel=5e-5)
    for n, u, v in zip(("dh", "de"), a[2:4], b[2:4]):
        assert_close(u, v, name=n, rtol=1e-3, arel=2e-4, l2=2e-3)
    for k in PMAP:
        assert_close(a[4][k], b[4][k], name=k, rtol=1e-3, arel=2e-4, l2=2e-3)


def test_training_in_kernel_random_mask_vs_oracle(gpu, egt_lib):
    from oracle import rng_ref
    B, N, nodes, p = 2, 48, [48, 40], 0.15
    inp, params = PB.make(B, N, nodes, seed=11)
    blk = _block(params, gpu, rand_p=p)
    blk.mha.random_mask_prob = p
    blk.train()
    out = _run(blk, inp, gpu, "library")
    m = blk.mha
    seed = (m.seed * 0x9E3779B97F4A7C15 + m._calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    inp2 = dict(inp, rand_mask=torch.from_numpy(rng_ref.random_mask(seed, B, N, 8, p)))
    _compare(out, CS.block_oracle(inp2, params, PB.ATTRS))


def test_no_clip(gpu, egt_lib):
    from egt_amd import EGTBlock
    inp, params = PB.make(1, 32, [27], seed=3)
    blk = EGTBlock(model_width=512, edge_width=32, num_heads=8, clip_logits_value=None, fused="auto").to(gpu).eval()
    with torch.no_grad():
        for k, (m, a) in PMAP.items():
            getattr(getattr(blk, m), a).copy_(params[k].to(gpu))
    out = _run(blk, inp, gpu, "library")
    _compare(out, CS.block_oracle(inp, params, dict(clip_logits_value=None, **PB.ATTRS)))


@pytest.mark.parametrize("recipe", [r for r in CD.BLOCK_RECIPES if CD.excluded("block", "pair_d64", r) is None])
def test_conditioning(recipe, gpu, egt_lib):
    """tests/test_conditioning_cpu.py holds the fairness of these (case, recipe) pairs"""
    case = CD.make_block("pair_d64", recipe)
    inp = case["inp"]
    mod, _ = CD.block_modules(case, gpu, fused="auto")
    h2, e2, dh, de, grads = _run(mod, inp, gpu, "library")
    got = dict(h_out=h2, e_out=e2, dh=dh, de=de)
    got.update({f"L0.{k}": g for k, g in grads.items()})
    CD.compare(got, CD.block_oracle(case), case)


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.add(func.overloadpacket.__name__ if hasattr(func, "overloadpacket") else str(func))
        return func(*args, **(kwargs or {}))


BANNED = {"mm", "addmm", "matmul", "bmm", "native_layer_norm", "native_layer_norm_backward", "sum"}


def test_launches_and_no_torch_math(gpu, egt_lib):
    inp, params = PB.make(2, 48, [48, 31], seed=5)
    blk = _block(params, gpu).eval()
    _run(blk, inp, gpu, "library")                      # (lazy one-time work first)
    buf = C.create_string_buffer(8192)
    seen = {}
    for node in ("library", "torch"):
        egt_lib.egt_prof_filter(b""); egt_lib.egt_prof_enable(2)
        try:
            with _Recorder() as rec:
                _run(blk, inp, gpu, node)
            torch.cuda.synchronize()
        finally:
            egt_lib.egt_prof_enable(0)
        egt_lib.egt_prof_names(buf, 8192)
        seen[node] = (set(buf.value.decode().split()), rec.ops)
    names, ops = seen["library"]
    assert KERNELS <= names and {"k_pair_fwd", "k_pair_bwd", "k_attn_mfma_bwd_q"} <= names, names
    assert not BANNED & ops, sorted(BANNED & ops)
    names_t, ops_t = seen["torch"]                      # the instrument sees the torch node side, backward included
    assert not KERNELS & names_t and {"k_pair_fwd", "k_pair_bwd"} <= names_t, names_t
    assert {"native_layer_norm", "native_layer_norm_backward"} <= ops_t and {"mm", "addmm"} & ops_t, sorted(ops_t)


def test_last_path_is_fused_pair_on_either_route(gpu, egt_lib, monkeypatch):
    from egt_amd import pair
    inp, params = PB.make(1, 37, [29])
    blk = _block(params, gpu).eval()
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(pair, "_PAIR_NODE", on)     # the remembered answer of the process switch
        with torch.no_grad():
            outs[on] = blk(inp["h"].to(gpu), inp["e"].to(gpu), inp["mask"].to(gpu))
        assert blk.last_path == "fused-pair"
    with torch.no_grad():
        forced = pair.block_pair(blk, inp["h"].to(gpu), inp["e"].to(gpu), inp["mask"].to(gpu), node="library")
    assert torch.equal(outs[True][0], forced[0]) and torch.equal(outs[True][1], forced[1])
    assert_close(outs[True][0], outs[False][0], name="h_out", rtol=1e-4, arel=5e-5)
    with pytest.raises(ValueError):
        pair.block_pair(blk, inp["h"].to(gpu), inp["e"].to(gpu), inp["mask"].to(gpu), node="vendor")


def test_capture_replays_bit_equal(gpu, egt_lib):
    """forward + backward of the library route (random mask off) in one hipGraph on one stream: three replays == eager"""
    from egt_amd import GraphedStep
    from egt_amd.pair import block_pair
    B, N, nodes = 5, 32, [32, 17, 1, 32, 20]
    inp, params = PB.make(B, N, nodes)
    ref = _block(params, gpu).eval()
    want = _run(ref, inp, gpu, "library")
    blk = copy.deepcopy(ref)
    h = inp["h"].to(gpu).requires_grad_(); e = inp["e"].to(gpu).requires_grad_()
    mask, dh, de = inp["mask"].to(gpu), inp["dh"].to(gpu), inp["de"].to(gpu)

    def step():
        h.grad = None; e.grad = None
        for p in blk.parameters():
            p.grad = None
        h2, e2 = block_pair(blk, h, e, mask, node="library")
        torch.autograd.backward([h2, e2], [dh, de])
        return h2.detach(), e2.detach()
    g = GraphedStep(step, None, warmup=2)
    for k in range(3):
        h2, e2 = g.replay()
        torch.cuda.synchronize()
        got = (h2.clone(), e2.clone(), h.grad.clone(), e.grad.clone(), {n: t.clone() for n, t in _grads(blk).items()})
        _same(want, got, f"replay {k + 1} vs eager")
        for t in (h2, e2, h.grad, e.grad, *_grads(blk).values()):
            t.fill_(float("nan"))                       # the next replay rewrites every result


def test_gradients_land_in_flat_sinks(gpu, egt_lib):
    from egt_amd import fused
    from egt_amd.dp import FlatGradAllReduce
    inp, params = PB.make(1, 37, [29])
    plain = _block(params, gpu).eval()
    want = _run(plain, inp, gpu, "library")
    blk = copy.deepcopy(plain)
    plist = list(blk.parameters())
    fa = FlatGradAllReduce(plist, direct=True)
    fa.zero(); fa.rebind()
    _, rets = fused.grad_sinks(plist)
    assert all(r is None for r in rets), "autograd receives None for every pre-bound view"
    fa.flat.fill_(float("nan"))
    from egt_amd.pair import block_pair
    hg = inp["h"].to(gpu).requires_grad_(); eg = inp["e"].to(gpu).requires_grad_()
    h2, e2 = block_pair(blk, hg, eg, inp["mask"].to(gpu), node="library")
    torch.autograd.backward([h2, e2], [inp["dh"].to(gpu), inp["de"].to(gpu)])
    off = 0
    for p in plist:                                     # .grad still aliases the flat buffer: the kernels wrote into it
        assert p.grad.data_ptr() == fa.flat[off:].data_ptr()
        off += p.numel()
    assert off == fa.flat.numel() and bool(torch.isfinite(fa.flat).all())
    assert torch.equal(hg.grad, want[2]) and torch.equal(eg.grad, want[3])
    for k, g in _grads(blk).items():
        assert torch.equal(g, want[4][k]), k
