"""The launch plane of the three kernels that close egt_stack_bwd -- TEST INFRASTRUCTURE shared by
tests/test_stack_tail_cpu.py and tests/test_stack_tail_gpu.py (no test functions here).

    k_node_wgrads        dWqkv / dWo of every layer, grid = (row chunks, layers)
    k_sum_segments       reduces every per-workgroup partial (7 segments per layer)
    k_edge_param_grads   finishes the edge-parameter gradients, one workgroup per layer

plan_tail() restates the host rules that shape them, from B * N, the layer count and the backward's workgroup count TOGETHER:

    plan_for                    egt_amd/csrc/egt_block.hip   TL (query rows per backward workgroup), NLR = ceil(N / TL),
                                                             nwg_bwd = B * NLR = edge-parameter partials per layer, the family
    wgrad_rows_per_wg           egt_amd/csrc/egt_node.hip    128 rows per workgroup, or more in whole 32-row steps when
                                                             chunks x layers would leave one round of 2 x CUs workgroups
    egt_node_launch_reduce      egt_amd/csrc/egt_node.hip    k_sum_segments in launches of 11 layers (77 segments),
                                                             k_edge_param_grads in launches of 16 layers
    egt_node_launch_pre_stack   egt_amd/csrc/egt_node.hip    the forward's edge-weight preparation: k_node_pre_stack<16>, <40>,
                                                             or k_edge_prep above 40 layers

and classifies a partial count np by the path k_sum_segments (8 lane groups pg, 8 loads per round, 64 partials a full round)
takes through its two loops:

    idle           np < 8              lane groups np .. 7 load nothing
    partial        8 <= np <= 56       the partial round only
    mixed          57 <= np <= 63      lane groups pg < np - 56 run a full round and no partial one, the others the partial one
    full           np % 64 == 0        full rounds only
    full+partial   otherwise           full rounds, then the partial round

The library's own answers (egt_stack_tail_form, egt_block_launch_form: both need no device) are held to plan_tail() by the CPU
test, so the GPU test's expectations do not rest on this restatement alone.
"""
import ctypes as C
import functools
import math
import os
import re
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CUS = 256                      # egt_device_cus(): the MI355X's, and the fallback of a process without a device
WG_ROWS, STEP = 128, 32        # egt_node.hip: WG_ROWS, the 32-row step of k_node_wgrads
SUM_G, SUM_U = 8, 8            # k_sum_segments: lane groups, loads per lane and round
SUM_LAYERS, EPG_LAYERS = 11, 16
PRE_STACK = (16, 40)           # layer slots of the two k_node_pre_stack instances
MAX_LAYERS = 64                # the C ABI's limit of a stack call
H = 8

FWD_TOL = dict(rtol=2e-4, arel=5e-5)     # h', e' of tests/test_block_gpu.py::test_stack_call_vs_oracle
CAP = 0.25                               # tests/conditioning.py: the fairness cap

NAMES = {"norm_edge.gamma": ("norm_edge", "gamma"), "norm_edge.beta": ("norm_edge", "beta"),
         "attention_gates.kernel": ("attention_gates", "kernel"), "attention_gates.bias": ("attention_gates", "bias"),
         "dense_edge_b.kernel": ("dense_edge_b", "kernel"), "dense_edge_b.bias": ("dense_edge_b", "bias"),
         "norm_mha.gamma": ("norm_mha", "gamma"), "norm_mha.beta": ("norm_mha", "beta"),
         "dense_qkv.kernel": ("dense_qkv", "kernel"), "dense_qkv.bias": ("dense_qkv", "bias"),
         "dense_mha.kernel": ("dense_mha", "kernel"), "dense_mha.bias": ("dense_mha", "bias"),
         "dense_edge_r.kernel": ("dense_edge_r", "kernel"), "dense_edge_r.bias": ("dense_edge_r", "bias")}
WGRAD_PARAMS = ("dense_qkv.kernel", "dense_mha.kernel")      # what k_node_wgrads produces


def _cdiv(a, b):
    return (a + b - 1) // b


def sum_class(np_):
    """the path of k_sum_segments for np_ partials (module docstring)"""
    full = SUM_G * SUM_U
    if np_ < SUM_G:
        return "idle"
    if np_ <= full - SUM_G:
        return "partial"
    if np_ < full:
        return "mixed"
    return "full" if np_ % full == 0 else "full+partial"


def plan_tail(B, N, De, Dh, layers, cus=CUS):
    """dict(TL, NLR, nwg_bwd, bwd, bwd_form, rows_per_wg, steps, chunks, last_chunk_rows, last_step_rows, d64, edge_class,
    weight_class, reduce_launches, epg_launches, prep, edge_prep, tail_form) for an fp32 stack call without a mask tensor."""
    assert 1 <= layers <= MAX_LAYERS and Dh % H == 0
    # ---- plan_for (egt_block.hip): the backward's row groups
    groups = _cdiv(N, 16)
    tg = 2 * cus // B
    tg = min(tg, _cdiv(N, 4) if B * _cdiv(N, 4) <= cus else _cdiv(N, 8))
    if De != 8:
        TL = _cdiv(N, max(tg, groups))
    elif B * groups <= cus:
        TL = 16
        if N > 8:
            TL = next((tl for tl in range(8, 16) if B * _cdiv(N, tl) <= cus), 16)
    else:
        TL = _cdiv(N, groups)
    NLR = _cdiv(N, TL)
    nwg = B * NLR
    if De == 8:
        bwd, nw = "k_narrow_bwd", (8 if nwg <= cus and N >= 64 else 4)
    elif De <= 16:
        bwd, nw = "k_block_bwd_v4r", 4
    else:
        bwd, nw = "k_block_bwd_v5", 4
    # ---- wgrad_rows_per_wg (egt_node.hip)
    rows = B * N
    per_layer = max(1, 2 * cus // layers)
    rpw = max(WG_ROWS, _cdiv(_cdiv(rows, per_layer), STEP) * STEP)
    chunks = _cdiv(rows, rpw)
    last_chunk = rows - (chunks - 1) * rpw
    last_step = last_chunk - (_cdiv(last_chunk, STEP) - 1) * STEP
    # ---- egt_node_launch_reduce, egt_node_launch_pre_stack (egt_node.hip)
    prep = "stack16" if layers <= PRE_STACK[0] else "stack40" if layers <= PRE_STACK[1] else "edge_prep"
    P = dict(TL=TL, NLR=NLR, nwg_bwd=nwg, bwd=bwd, bwd_form=f"{bwd}/{nw}w/tl{TL}",
             rows_per_wg=rpw, steps=rpw // STEP, chunks=chunks, last_chunk_rows=last_chunk, last_step_rows=last_step, d64=Dh == 64,
             edge_class=sum_class(nwg), weight_class=sum_class(chunks),
             reduce_launches=_cdiv(layers, SUM_LAYERS), epg_launches=_cdiv(layers, EPG_LAYERS), prep=prep, edge_prep=prep == "edge_prep")
    P["tail_form"] = (f"wgrad={rpw}r/{chunks}c partials={nwg} reduce={P['reduce_launches']} epg={P['epg_launches']} prep={prep}")
    return P


# (B, N, De, Dh, layers): the class the row is there for, as plan_tail() fields that must hold.  test_stack_tail_cpu.py checks
# every annotation against plan_tail() and plan_tail() against the library.
ROWS = {
    # five steps, 27 chunks, a two-step last chunk; 384 = 6 x 64 partials; exactly EPG_LAYERS layers; two reduce launches
    (128, 33, 8, 64, 16): dict(rows_per_wg=160, steps=5, chunks=27, last_chunk_rows=64, last_step_rows=32, nwg_bwd=384,
                               edge_class="full", weight_class="partial", epg_launches=1, reduce_launches=2, prep="stack16",
                               bwd="k_narrow_bwd"),
    # 7 chunks: idle lane groups on the weight partials; a 24-row last step; 144 = 2 x 64 + 16; the k_edge_prep fallback
    (36, 30, 64, 64, 58): dict(rows_per_wg=160, chunks=7, weight_class="idle", last_chunk_rows=120, last_step_rows=24, nwg_bwd=144,
                               edge_class="full+partial", reduce_launches=6, epg_launches=4, edge_prep=True, bwd="k_block_bwd_v5"),
    # the headline's six steps; an 8-row last step; the ABI's 64-layer limit
    (44, 30, 16, 64, 64): dict(rows_per_wg=192, steps=6, chunks=7, last_chunk_rows=168, last_step_rows=8, nwg_bwd=176,
                               edge_class="full+partial", reduce_launches=6, epg_launches=4, edge_prep=True, bwd="k_block_bwd_v4r"),
    # Dh = 48 (d = 6): k_node_wgrads<false> under the five-step walk; k_node_pre_stack<40> at its limit
    (50, 31, 48, 48, 40): dict(d64=False, rows_per_wg=160, chunks=10, last_chunk_rows=110, last_step_rows=14, nwg_bwd=200,
                               edge_class="full+partial", weight_class="partial", prep="stack40", reduce_launches=4, epg_launches=3),
    # 60 partials: lane groups 0..3 take a full round, 4..7 only the partial one
    (5, 48, 64, 64, 3): dict(nwg_bwd=60, edge_class="mixed", rows_per_wg=128, chunks=2, weight_class="idle", prep="stack16"),
    # 77 segments in one k_sum_segments launch, then 11 + 1 layers in two
    (2, 16, 64, 64, 11): dict(reduce_launches=1, epg_launches=1, rows_per_wg=128, chunks=1, edge_class="partial"),
    (2, 16, 64, 64, 12): dict(reduce_launches=2, epg_launches=1, rows_per_wg=128, chunks=1, edge_class="partial"),
}
# the rows that run again through the guarded arenas of tests/memcontract.py (the 128-graph row, the 64-layer row)
MEMCONTRACT_ROWS = ((128, 33, 8, 64, 16), (44, 30, 16, 64, 64))


def row_id(row):
    B, N, De, Dh, Ly = row
    return f"b{B}_n{N}_de{De}_dh{Dh}_ly{Ly}"


# B = 2, Ly = 3 shapes of tests/test_block_gpu.py::test_stack_call_vs_oracle, as (B, N, De, Dh, layers): what the suite held
# against the oracle before this table (the CPU test holds plan_tail() to the library at these too)
EXISTING = [(2, N, De, Dh, 3) for N, De, Dh in ((24, 64, 64), (32, 64, 64), (11, 48, 48), (20, 8, 64), (80, 16, 64), (32, 32, 64),
                                                (48, 48, 64), (32, 8, 64), (128, 8, 64), (150, 8, 64), (144, 16, 64), (150, 16, 64),
                                                (37, 48, 48), (40, 8, 32), (24, 16, 40), (20, 64, 8), (40, 64, 64), (150, 64, 64))]


def desc(row):
    """the egt_block_desc of a row's eval-mode stack call (what egt_amd.fused._desc builds for it)"""
    from egt_amd import _lib as L
    B, N, De, Dh, _ = row
    return L.BlockDesc(B=B, N=N, H=H, d=Dh // H, De=De, dtype=L.EGT_F32, flags=L.BF_GATE | L.BF_CLIP, clip_lo=-5.0, clip_hi=5.0,
                       random_mask_prob=0.0, ln_eps=1e-3, reserved=0, seed=0, seed_device=None)


def library_forms(lib, row):
    """(egt_stack_tail_form, the backward part of egt_block_launch_form) for a row"""
    d = desc(row)
    tail = lib.egt_stack_tail_form(C.byref(d), row[4])
    form = lib.egt_block_launch_form(C.byref(d))
    assert tail is not None and form is not None, row
    return tail.decode(), re.search(r"bwd=(\S+)", form.decode()).group(1)


# ---------------------------------------------------------------------------------------------- inputs and the oracle ----
@functools.lru_cache(maxsize=None)
def make_inputs(row):
    """Seeded host tensors of a row: randn h and e; graph 0 unpadded, the last graphs padded to n in [N/2, N]; randn upstream
    dh and de; per layer init_block_params(randomize_norm=True).  dict(h, e, mask, dh, de, layers: [{name: tensor}])."""
    from oracle import egt_oracle as O
    B, N, De, Dh, Ly = row
    g = torch.Generator().manual_seed(1000003 * B + 10007 * N + 101 * De + 7 * Dh + Ly)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    h, e = r(B, N, Dh), r(B, N, N, De)
    n = torch.full((B,), N, dtype=torch.int64)
    padded = max(1, B // 4)                                     # the last quarter of the batch
    n[B - padded:] = torch.randint(N // 2, N, (padded,), generator=g)   # (N itself left out: every one of them IS padded)
    n[0] = N
    mask = torch.arange(N)[None, :] < n[:, None]
    dh, de = r(B, N, Dh), r(B, N, N, De)
    layers = [O.init_block_params(Dh, De, H, dtype=torch.float32, generator=g, randomize_norm=True) for _ in range(Ly)]
    return dict(h=h, e=e, mask=mask, dh=dh, de=de, layers=layers)


def run_oracle(row, dtype):
    """O.stack_forward and its gradients in `dtype` on the CPU: dict(h_out, e_out, dh, de, params: [{name: grad}])"""
    from oracle import egt_oracle as O
    inp = make_inputs(row)
    h = inp["h"].to(dtype).requires_grad_(); e = inp["e"].to(dtype).requires_grad_()
    layers = [{k: v.to(dtype).requires_grad_() for k, v in lp.items()} for lp in inp["layers"]]
    ho, eo = O.stack_forward(h, e, inp["mask"], layers, num_heads=H)
    flat = [t for lp in layers for t in lp.values()]
    gr = torch.autograd.grad([ho, eo], [h, e] + flat, [inp["dh"].to(dtype), inp["de"].to(dtype)])
    gi = iter(gr[2:])
    return dict(h_out=ho.detach(), e_out=eo.detach(), dh=gr[0], de=gr[1], params=[{k: next(gi) for k in lp} for lp in layers])


@functools.lru_cache(maxsize=None)
def oracle(row):
    """the fp64 oracle of a row, computed once per process and shared (callers must not modify it)"""
    return run_oracle(row, torch.float64)


def tensors(res):
    """[(name, tensor, is_grad)] of a run_oracle()-shaped result, parameters named L<layer>.<parameter>"""
    out = [("h_out", res["h_out"], False), ("e_out", res["e_out"], False), ("dh", res["dh"], True), ("de", res["de"], True)]
    for li, lp in enumerate(res["params"]):
        out += [(f"L{li}.{k}", lp[k], True) for k in NAMES]
    return out


def margins(got, ref):
    """{name: worst |error| / tolerance} of every tensor under the GPU test's tolerances (util.margin's model; an
    analytically-zero reference is measured against BWD's zero_atol)"""
    from util import BWD, margin
    out = {}
    for (name, a, is_grad), (_, r, _) in zip(tensors(got), tensors(ref)):
        if is_grad and float(r.abs().max()) < 1e-9:
            out[name] = float((a.double().cpu() - r.double().cpu()).abs().max()) / BWD["zero_atol"]
            continue
        tol = dict(rtol=BWD["rtol"], arel=BWD["arel"]) if is_grad else FWD_TOL
        out[name] = margin(a, r, **tol)
    return out


# ------------------------------------------------------------------------------------------------------------ the GPU ----
def build_stack(row, dev):
    """EGTStack(fused=True) in eval mode with the row's parameters"""
    from egt_amd import EGTStack
    B, N, De, Dh, Ly = row
    st = EGTStack(model_height=Ly, model_width=Dh, edge_width=De, num_heads=H, fused=True).to(dev).eval()
    with torch.no_grad():
        for blk, lp in zip(st.blocks, make_inputs(row)["layers"]):
            for k, (m, a) in NAMES.items():
                getattr(getattr(blk, m), a).copy_(lp[k].to(dev))
    return st


def run_gpu(st, row, dev):
    """one forward and backward of the row through the one-call stack: a run_oracle()-shaped result"""
    inp = make_inputs(row)
    for p in st.parameters():
        p.grad = None
    h = inp["h"].to(dev).requires_grad_(); e = inp["e"].to(dev).requires_grad_()
    h2, e2 = st(h, e, inp["mask"].to(dev))
    assert st.last_path == "fused-stack", st.last_path
    torch.autograd.backward([h2, e2], [inp["dh"].to(dev), inp["de"].to(dev)])
    torch.cuda.synchronize()
    params = [{k: getattr(getattr(blk, m), a).grad.clone() for k, (m, a) in NAMES.items()} for blk in st.blocks]
    return dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad, params=params)


def launch_counts(lib, fn):
    """run fn() under the C ABI's launch profiler: (fn's result, {kernel name: launches})"""
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.egt_prof_enable(0)
    buf = C.create_string_buffer(4096)
    lib.egt_prof_names(buf, 4096)
    count = {}
    for name in buf.value.decode().split():
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(name.encode(), C.byref(cnt), C.byref(ms))
        if cnt.value:
            count[name] = cnt.value
    return out, count


if __name__ == "__main__":      # the fairness figures of every row (DESIGN.md records them)
    import time
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for row_ in ROWS:
        t0 = time.time()
        m = margins(run_oracle(row_, torch.float32), oracle(row_))
        worst = max(m, key=m.get)
        print(f"{row_id(row_)}: fp32 oracle worst margin {m[worst]:.4f} ({worst}); {time.time() - t0:.1f} s", flush=True)
