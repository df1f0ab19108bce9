"""The cross-talk FFN's edge side (egt_xtalk_fwd / egt_xtalk_bwd) across its launch plane against the fp64 reference:
every row of tests/xtalk_plane.py -- all fifteen <W, SNT> instances per direction, the split positions, N from 1 to 150, the
backward's grown row blocks, non-prefix masks -- under xtalk_plane.hold (e' as its update, hn, d_e, d_hr, d_hc and the six
parameter gradients; util.FWD / util.BWD unchanged).  tests/test_xtalk_plane_cpu.py holds the library's plan to the restatement
the rows are chosen by, and the comparison to fairness.  Each row first asserts that the library plans the launch the row is
there for (egt_xtalk_launch_form).
EGT_XTALK_PLANE_MARGINS=<path>: the worst error / tolerance of every row is written there (JSON) when the module ends
(profiles/xtalk_plane_margins.json is such a dump)."""
import ctypes as C
import json
import os

import pytest
import torch

import xtalk_plane as XP

pytestmark = pytest.mark.gpu
MARGINS = {}
ROWS = XP.all_rows()
IDS = [XP.row_id(*r) for r in ROWS]


@pytest.fixture(scope="module", autouse=True)
def _dump_margins():
    yield
    path = os.environ.get("EGT_XTALK_PLANE_MARGINS")
    if path and MARGINS:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(tolerance="util.FWD (e_out as its update e' - e, hn) / util.BWD (gradients) under xtalk_plane.hold; "
                                     "margin = worst |error| / tolerance (< 1 passes)",
                           worst_margin=MARGINS), f, indent=1, sort_keys=True)


def _assert_form(row, act, egt_lib):
    B, N, De, Dh, s_e, s_n = row[:6]
    form = egt_lib.egt_xtalk_launch_form(C.byref(XP.desc(row, act)))
    assert form is not None and form.decode() == XP.launch_form(B, N, De, s_e, s_n), form


@pytest.mark.parametrize("table,i,row", ROWS, ids=IDS)
def test_row_vs_fp64_reference(table, i, row, gpu, egt_lib):
    act = XP.row_act(table, i, row)
    _assert_form(row, act, egt_lib)
    got = XP.edge_gpu(row, act, gpu)
    ref = XP.edge_reference(row, act)
    e = XP.edge_inputs(row)[0]["e"]
    name = XP.row_id(table, i, row)
    sink = {}
    try:
        XP.hold(got, ref, e, check=False, sink=sink)            # measure first: a failing row still reports its margin
    finally:
        if sink:
            top = max(sink, key=sink.get)
            MARGINS[name] = dict(worst=round(sink[top], 4), where=top)
            print(f"[xtalk plane] {name}: worst margin {sink[top]:.4f} on {top}")
    XP.hold(got, ref, e, name=name)
    if table == "MASKS":
        empty = [b for b, n in enumerate(row[7]) if n == 0]
        assert empty
        for k in ("hn", "d_e", "d_hr"):
            for b in empty:
                zero = ref[k][b] == 0
                assert bool((got[k][b].cpu()[zero] == 0).all()), f"{k}: graph {b} has no node, the reference is exactly 0 here"
        assert bool((ref["hn"][empty[0]] == 0).all())           # (divide_no_nan: the whole exchange of an empty graph)
        assert all(bool(torch.isfinite(t).all()) for t in got.values())


@pytest.mark.parametrize("row", XP.TWICE, ids=[f"B{r[0]}_N{r[1]}_De{r[2]}" for r in XP.TWICE])
def test_two_runs_are_bit_equal(row, gpu, egt_lib):
    """no atomics: the grown row blocks, the workgroup partials and their sums come out in one order"""
    a, b = XP.edge_gpu(row, "elu", gpu), XP.edge_gpu(row, "elu", gpu)
    for k in a:
        assert torch.equal(a[k], b[k]), k
