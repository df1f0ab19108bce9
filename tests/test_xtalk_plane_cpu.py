"""The cross-talk FFN's launch plane pinned without a GPU: the library's own answers (egt_xtalk_workspace_bytes,
egt_xtalk_launch_form: both pure host functions of the descriptor) against the restatement tests/xtalk_plane.plan for every
row of the tables that tests/test_xtalk_plane_gpu.py runs, what the tables reach (all fifteen <W, SNT> instances per direction,
the backward's grown row blocks), and the FAIRNESS of the comparison: the same reference code in fp32 on the CPU stays within
conditioning.CAP = 0.25 of util.FWD / util.BWD under xtalk_plane.hold on every row."""
import ctypes as C
import re

import pytest
import torch

import conditioning as CD
import xtalk_plane as XP

ROWS = XP.all_rows()
IDS = [XP.row_id(*r) for r in ROWS]


@pytest.fixture(autouse=True)
def _one_thread():
    """the fp32 oracle's summation order (and with it the measured margin) must not depend on the machine's core count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("table,i,row", ROWS, ids=IDS)
def test_workspace_and_launch_form_equal_the_restated_plan(table, i, row, egt_lib):
    B, N, De, Dh, s_e, s_n = row[:6]
    d = XP.desc(row, XP.row_act(table, i, row))
    p = XP.plan(B, N, De, s_e, s_n)
    assert egt_lib.egt_xtalk_supported(C.byref(d)) == 1
    assert egt_lib.egt_xtalk_workspace_bytes(C.byref(d)) == 4 * p.total
    form = egt_lib.egt_xtalk_launch_form(C.byref(d)).decode()
    assert form == XP.launch_form(B, N, De, s_e, s_n)
    m = re.fullmatch(r"fwd=k_xtalk_fwd<(\d+),(\d)>/rb(\d+)/g(\d+) bwd=k_xtalk_bwd<(\d+),(\d)>/rb(\d+)/g(\d+)(/walk2)?", form)
    assert m, form
    got = tuple(int(x) for x in m.groups()[:8]) + (m.group(9) is not None,)
    assert got == (p.W, p.snt, p.rb_f, B * p.wpg_f, p.W, p.snt, p.rb_b, B * p.wpg_b, p.walk2)
    # the plan's own invariants: every row belongs to exactly one row block, every row block to one wave of one workgroup
    for rb, nblk, wpg in ((p.rb_f, p.nblk_f, p.wpg_f), (p.rb_b, p.nblk_b, p.wpg_b)):
        assert (nblk - 1) * rb < N <= nblk * rb and 4 * (wpg - 1) < nblk <= 4 * wpg


def test_the_tables_reach_every_instance_in_both_directions():
    seen = {(p.W, p.snt) for _, _, r in ROWS for p in [XP.plan(r[0], r[1], r[2], r[4], r[5])]}
    assert seen == {(W, s) for W in (16, 32, 64) for s in range(5)}
    inst = {(r[2], (r[5] + 15) // 16) for r in XP.INSTANCES}
    assert inst == seen and all(r[5] % 16 for r in XP.INSTANCES if r[5])      # every last exchange tile is partial
    walk2 = {(p.W, p.snt) for _, _, r in ROWS for p in [XP.plan(r[0], r[1], r[2], r[4], r[5])] if p.walk2}
    assert walk2 == {(64, 3), (64, 4)}


def test_growth_rows_reach_the_grown_row_blocks():
    got = [(p.rb_b, p.nblk_b, p.wpg_b) for r in XP.GROWTH for p in [XP.plan(r[0], r[1], r[2], r[4], r[5])]]
    assert got == [(16, 3, 1), (24, 1, 1), (16, 5, 2)]
    assert all(XP.plan(r[0], r[1], r[2], r[4], r[5]).rb_b == 8 for t, _, r in ROWS if t != "GROWTH")
    # the configuration the growth exists for: B = 128 at N = 150 would take 640 workgroups at 8 rows per wave
    p = XP.plan(128, 150, 16, 4, 16)
    assert (p.rb_b, p.nblk_b, p.wpg_b) == (16, 10, 3)


@pytest.mark.parametrize("B,N,rows,grid", [(512, 19, 8, 512), (513, 19, 24, 513), (256, 37, 8, 512), (257, 37, 16, 257),
                                           (128, 128, 8, 512), (129, 128, 16, 258), (600, 8, 8, 600), (600, 16, 16, 600),
                                           (600, 17, 24, 600), (171, 65, 16, 342), (170, 65, 8, 510)])
def test_growth_boundaries(B, N, rows, grid, egt_lib):
    """both sides of each comparison of the growth loop, by hand (plan only: none of these runs on the GPU): exactly 512 workgroups
    stay at 8 rows per wave, 513 grow; the growth ends at the first row block that holds the whole graph"""
    from egt_amd.xtalk import _desc
    p = XP.plan(B, N, 16, 4, 16)
    assert (p.rb_b, B * p.wpg_b) == (rows, grid)
    d = _desc(B, N, 16, 64, 4, 16, "elu")
    assert egt_lib.egt_xtalk_launch_form(C.byref(d)).decode() == XP.launch_form(B, N, 16, 4, 16)
    assert f"bwd=k_xtalk_bwd<16,1>/rb{rows}/g{grid}" in XP.launch_form(B, N, 16, 4, 16)
    assert egt_lib.egt_xtalk_workspace_bytes(C.byref(d)) == 4 * p.total


def test_sizes_reach_idle_waves_and_many_workgroups():
    plans = {r[1]: XP.plan(r[0], r[1], r[2], r[4], r[5]) for r in XP.SIZES if r[2] == 16}
    assert plans[1].nblk_f == 1 and plans[8].nblk_f == 1 and plans[9].nblk_f == 2          # three / two waves without a row block
    assert plans[33].wpg_f == 2 and plans[33].nblk_f == 5                                   # the last workgroup: one live wave
    assert plans[65].wpg_f == 3 and plans[150].wpg_f == 5 and plans[150].nblk_f == 19
    assert {n for n in plans if n % 16 == 0} == {16, 32, 64}                                # no ragged tile


def test_masks_row_holds_the_four_kinds():
    m = XP.row_mask(XP.MASKS[0])
    assert m[0].all() and not m[3].any() and m[2].nonzero().flatten().tolist() == [20]
    assert m[1].tolist() == [i % 3 != 1 for i in range(21)]


@pytest.mark.parametrize("table,i,row", ROWS, ids=IDS)
def test_fp32_reference_is_within_the_cap(table, i, row):
    act = XP.row_act(table, i, row)
    sink = {}
    worst = XP.hold(XP.edge_oracle_fp32(row, act), XP.edge_reference(row, act), XP.edge_inputs(row)[0]["e"], check=False, sink=sink)
    top = max(sink, key=sink.get)
    assert worst <= CD.CAP, f"the fp32 reference reaches {worst:.3f} of the tolerance on {top} (cap {CD.CAP})"


def test_a_declined_descriptor_gets_no_plan(egt_lib):
    from egt_amd.xtalk import _desc
    for d in (_desc(2, 9, 48, 48, 12, 12, "elu"), _desc(2, 9, 16, 64, 6, 16, "elu"), _desc(2, 9, 16, 64, 0, 0, "elu"),
              _desc(2, 9, 16, 64, 16, 0, "relu"), _desc(2, 0, 16, 64, 4, 16, "elu"),
              _desc(2, 9, 16, 64, 4, 16, "elu", dtype=torch.bfloat16)):
        assert egt_lib.egt_xtalk_supported(C.byref(d)) == 0
        assert egt_lib.egt_xtalk_launch_form(C.byref(d)) is None
        assert egt_lib.egt_xtalk_workspace_bytes(C.byref(d)) == 0
    assert egt_lib.egt_xtalk_launch_form(None) is None
