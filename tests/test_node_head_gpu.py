"""Fused node-classification head on the GPU (egt_node_head_fwd / egt_node_head_bwd): stats and every gradient against fp64
autograd of the restatement (node_head_ref.py) and against the composed head on the GPU; masks, determinism, hipGraph capture
and direct gradient sinks."""
import pytest
import torch

import node_head_ref as NR
from util import assert_close, FWD, BWD

pytestmark = pytest.mark.gpu

S_UP = 0.7                                  # a non-unit upstream gradient of stats[0]
# (W, width -> hidden widths, C, activation, LayerNorm, B, N)
CASES = [(64, 64, 6, "elu", True, 3, 19), (64, 64, 2, "elu", True, 3, 19), (48, 48, 6, "relu", True, 3, 19),
         (16, 64, 3, "elu", False, 3, 19),
         (64, 64, 6, "elu", True, 2, 16),    # nothing masked, every tile full
         (64, 64, 6, "elu", True, 4, 70),    # 280 rows = 18 tiles -> 18 // 4 = 4 workgroups of 5, 5, 5, 3 tiles (NR.workgroups)
         (32, 64, 6, "elu", True, 3, 19)]    # W = 32: the two-tile instance of the shared tile body
_REF = {}


def _reference(case):
    """fp64 autograd of the restatement: computed once per case, shared, never modified"""
    if case not in _REF:
        W, width, Cn, act, ln, B, N = case
        x = NR.make_inputs(B, N, W, Cn)
        params = NR.head_params(W, width, Cn, ln)
        h64 = x["h"].double().requires_grad_()
        p64 = tuple(None if p is None else p.double().requires_grad_() for p in params)
        st, z = NR.ref_stats(h64, x["target"], x["mask"], x["class_weights"].double(), p64, act)
        gr = torch.autograd.grad(st[0] * S_UP, [h64] + [p for p in p64 if p is not None])
        _REF[case] = (x, params, dict(stats=st.detach(), d_h=gr[0], grads=list(gr[1:]), gap=NR.top2_gap(z.detach(), x["mask"])))
    return _REF[case]


def _run(fn, x, params, act, gpu, up=S_UP, target=None):
    h = x["h"].to(gpu).requires_grad_()
    ps = tuple(None if p is None else p.to(gpu).requires_grad_() for p in params)
    tgt = (x["target"] if target is None else target).to(gpu)
    st = fn(h, tgt, x["mask"].to(gpu), x["class_weights"].to(gpu), ps, act)
    (st[0] * up).backward()
    return dict(stats=st.detach(), d_h=h.grad, grads=[p.grad for p in ps if p is not None]), st


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_forward_backward(case, gpu, egt_lib):
    from egt_amd.node_head import node_head_loss, node_head_composed
    W, width, Cn, act, ln, B, N = case
    x, params, ref = _reference(case)
    assert ref["gap"] > 1e-3
    if (B, N) == (4, 70):
        assert NR.workgroups(B, N) == (4, 5) and NR.tile_census(x["mask"])[2] >= 3     # several workgroups; skipped tiles
    got, st = _run(node_head_loss, x, params, act, gpu)
    assert type(st.grad_fn).__name__ == "_FusedNodeHeadBackward"
    comp, _ = _run(node_head_composed, x, params, act, gpu)
    names = NR.NAMES if ln else NR.NAMES[2:]
    for other, tag in ((ref, "fp64"), (comp, "composed")):
        assert_close(got["stats"][0], other["stats"][0], name=f"loss sum vs {tag}", **FWD)
        assert got["stats"][1:].tolist() == other["stats"][1:].tolist(), f"hits and rows vs {tag}: exact"
        assert_close(got["d_h"], other["d_h"], name=f"d_h vs {tag}", **BWD)
        for n, a, r in zip(names, got["grads"], other["grads"]):
            assert_close(a, r, name=f"d {n} vs {tag}", **BWD)
    mask = x["mask"].to(gpu)
    assert float(got["stats"][2]) == float(x["mask"].sum())
    if not bool(mask.all()):
        assert float(got["d_h"][~mask].abs().max()) == 0.0, "exact zeros on masked rows"
    assert bool((got["d_h"][mask].abs().amax(-1) > 0).all()), "every unmasked row has a gradient"


def test_masked_targets_change_no_bit(gpu, egt_lib):
    from egt_amd.node_head import node_head_loss
    case = CASES[0]
    x, params, _ = _reference(case)
    a, _ = _run(node_head_loss, x, params, case[3], gpu)
    other = torch.where(x["mask"], x["target"], torch.full_like(x["target"], 2 ** 31 - 1))
    assert not torch.equal(other, x["target"]) and int(other[~x["mask"]].min()) > 16
    b, _ = _run(node_head_loss, x, params, case[3], gpu, target=other)
    neg = torch.where(x["mask"], x["target"], torch.full_like(x["target"], -(2 ** 31)))
    c, _ = _run(node_head_loss, x, params, case[3], gpu, target=neg)
    for o in (b, c):
        assert torch.equal(a["stats"], o["stats"]) and torch.equal(a["d_h"], o["d_h"])
        for p, q in zip(a["grads"], o["grads"]):
            assert torch.equal(p, q)


def test_upstream_gradient_scales_the_gradients(gpu, egt_lib):
    """the upstream gradient is read on the device; a power of two scales every gradient exactly"""
    from egt_amd.node_head import node_head_loss
    case = CASES[0]
    x, params, _ = _reference(case)
    one, _ = _run(node_head_loss, x, params, case[3], gpu, up=1.0)
    quarter, _ = _run(node_head_loss, x, params, case[3], gpu, up=-0.25)
    assert torch.equal(one["stats"], quarter["stats"])
    assert torch.equal(one["d_h"] * -0.25, quarter["d_h"]) and float(one["d_h"].abs().max()) > 0
    for p, q in zip(one["grads"], quarter["grads"]):
        assert torch.equal(p * -0.25, q)


@pytest.mark.parametrize("case", [CASES[0], CASES[5]], ids=["3x19", "4x70"])
def test_two_calls_are_bitwise_equal(case, gpu, egt_lib):
    from egt_amd.node_head import node_head_loss
    x, params, _ = _reference(case)
    a, _ = _run(node_head_loss, x, params, case[3], gpu)
    b, _ = _run(node_head_loss, x, params, case[3], gpu)
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["d_h"], b["d_h"])
    for p, q in zip(a["grads"], b["grads"]):
        assert torch.equal(p, q)


def test_graph_capture_replays_to_the_eager_bits(gpu, egt_lib):
    """forward + backward captured in a torch.cuda.graph (no host synchronisation inside: the upstream gradient is a device
    scalar); new inputs copied into the static tensors replay to what the eager call gives"""
    from egt_amd.node_head import node_head_loss
    case = CASES[5]
    W, width, Cn, act, ln, B, N = case
    x, params, _ = _reference(case)
    eager, _ = _run(node_head_loss, x, params, act, gpu)
    h = torch.zeros_like(x["h"], device=gpu).requires_grad_()
    ps = tuple(p.to(gpu).requires_grad_() for p in params)
    tgt, mask, cw = x["target"].to(gpu), x["mask"].to(gpu), x["class_weights"].to(gpu)

    def step():
        st = node_head_loss(h, tgt, mask, cw, ps, act)
        (st[0] * S_UP).backward()
        return st.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up outside the capture (on zeros)
    torch.cuda.current_stream().wait_stream(side)
    h.grad = None
    for p in ps:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = step()
    with torch.no_grad():
        h.copy_(x["h"].to(gpu))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st, eager["stats"]) and torch.equal(h.grad, eager["d_h"])
    for p, g in zip(ps, eager["grads"]):
        assert torch.equal(p.grad, g)


def test_gradients_land_in_bound_sinks(gpu, egt_lib):
    """FlatGradAllReduce(direct=True): the eight parameter gradients are written into their views of the flat buffer"""
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.node_head import node_head_loss
    case = CASES[0]
    x, params, _ = _reference(case)
    want, _ = _run(node_head_loss, x, params, case[3], gpu)
    ps = tuple(torch.nn.Parameter(p.to(gpu)) for p in params)
    ar = FlatGradAllReduce(list(ps), direct=True)
    ar.flat.fill_(float("nan"))                  # a sink is overwritten, not accumulated into
    ptrs = [p.grad.data_ptr() for p in ps]
    h = x["h"].to(gpu).requires_grad_()
    st = node_head_loss(h, x["target"].to(gpu), x["mask"].to(gpu), x["class_weights"].to(gpu), ps, case[3])
    (st[0] * S_UP).backward()
    assert [p.grad.data_ptr() for p in ps] == ptrs, "the gradients are the views of the flat buffer"
    for p, g in zip(ps, want["grads"]):
        assert torch.equal(p.grad, g)
    assert torch.equal(ar.flat, torch.cat([g.reshape(-1) for g in want["grads"]]))
    assert torch.equal(h.grad, want["d_h"])
