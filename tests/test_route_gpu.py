"""The route table of tests/test_fused_host_cpu.py run for real: one forward per configuration at the smallest ragged shapes
(B = 2, N = 19; N = 16 for the d = 64 pair operator), then what the block reports (last_path / last_edge_route)."""
import pytest
import torch

from test_fused_host_cpu import EDGE_DTYPE, ROUTE_CASES, make_block, static_edge_switch  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def run_case(case, dev):
    """one forward of the case's block; (last_path, last_edge_route) as the block reports them afterwards (None: not reported),
    or the name of the exception the forward raised"""
    torch.manual_seed(0)
    blk = make_block(case).to(dev)
    blk._static_ok = {}        # (the per-block dict this table was recorded with; unused since)
    B, N, H = 2, case["N"], blk.num_heads
    h = torch.randn(B, N, blk.model_width, device=dev)
    e = torch.randn(B, N, N, blk.edge_width, device=dev).to(EDGE_DTYPE[case["edge"]])
    mask = torch.ones(B, N, dtype=torch.bool, device=dev)
    mask[1, N - 3:] = False
    attn_mask = torch.zeros(B, N, N, H, device=dev) if case["attn_mask"] else None
    rand_mask = (torch.rand(B, N, N, H, device=dev) < 0.1) if case["rand_mask"] else None
    try:
        h2, e2 = blk(h, e, mask, attn_mask, rand_mask=rand_mask)
    except (RuntimeError, ValueError) as ex:
        return type(ex).__name__, getattr(blk, "last_path", None), getattr(blk, "last_edge_route", None)
    assert torch.isfinite(h2).all() and h2.shape == h.shape
    return getattr(blk, "last_path", None), getattr(blk, "last_edge_route", None)


def reported(case):
    """what a forward of the case reports, from the route the table pins"""
    if case["want"] is RuntimeError:
        return ("RuntimeError", None, None)
    if case["name"] == "constrained_no_mask":       # the composed path then refuses the call (the reference needs the mask too)
        return ("ValueError", "composed", None)
    if case["name"] == "none":                      # no edge channels: mha_block alone, nothing to route and nothing reported
        return (None, None)
    return case["want"]


@pytest.mark.parametrize("case", [c for c in ROUTE_CASES if c["name"] != "bf16_d64"], ids=lambda c: c["name"])
def test_route_for_real(gpu, egt_lib, static_edge_switch, case):
    static_edge_switch(case["no_static"])
    got = run_case(case, gpu)
    print(case["name"], got)
    assert got == reported(case)


def test_bf16_edges_at_d64_are_refused(gpu, egt_lib):
    """bf16 edge tensors exist on the fused block only, which does not cover d = 64: refused at construction"""
    from egt_amd import fused as FZ
    case = {c["name"]: c for c in ROUTE_CASES}["bf16_d64"]
    why = FZ.bf16_refusal(make_block(case).to(gpu))
    assert why is not None and "not covered by the fused block" in why
