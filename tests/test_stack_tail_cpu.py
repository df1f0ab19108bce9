"""The shape table of tests/stack_tail.py reaches the launch plane of egt_stack_bwd's closing kernels that it claims to, and the
comparison the GPU test makes at those shapes is fair (no GPU): every annotation equals plan_tail(); plan_tail() -- the restated
host rules -- equals what the library itself answers (egt_stack_tail_form, egt_block_launch_form) for every row and for the shapes
the older stack parity tests run; the rows cover every class of k_sum_segments, the long walk of k_node_wgrads with a partial
last step and with Dh < 64, and the layer counts at which a launch is cut; and the oracle's own code in fp32 on the CPU stays within
CAP of the tolerances the GPU test applies, for every tensor of every row."""
import ctypes as C

import pytest
import torch

import memcontract as M
import stack_tail as ST

ROWS = list(ST.ROWS)


@pytest.mark.parametrize("row", ROWS, ids=ST.row_id)
def test_rows_have_their_class(row):
    p = ST.plan_tail(*row)
    for k, v in ST.ROWS[row].items():
        assert p[k] == v, (row, k, p)
    B, N, _, _, Ly = row
    assert p["rows_per_wg"] % ST.STEP == 0 and p["rows_per_wg"] >= ST.WG_ROWS
    assert (p["chunks"] - 1) * p["rows_per_wg"] + p["last_chunk_rows"] == B * N and 0 < p["last_chunk_rows"] <= p["rows_per_wg"]
    assert 0 < p["last_step_rows"] <= ST.STEP and (p["last_chunk_rows"] - p["last_step_rows"]) % ST.STEP == 0
    # above WG_ROWS the rule holds the launch to one round of two workgroups per CU
    assert p["rows_per_wg"] == ST.WG_ROWS or p["chunks"] * Ly <= 2 * ST.CUS


@pytest.mark.parametrize("row", ROWS + ST.EXISTING, ids=ST.row_id)
def test_plan_tail_is_the_librarys_plan(row, egt_lib):
    p = ST.plan_tail(*row)
    tail, bwd = ST.library_forms(egt_lib, row)
    assert tail == p["tail_form"], (row, tail, p["tail_form"])
    assert bwd == p["bwd_form"], (row, bwd, p["bwd_form"])
    assert egt_lib.egt_block_bwd_kernel(C.byref(ST.desc(row))).decode() == p["bwd"]


def test_tail_form_answers_null_outside_the_cover(egt_lib):
    from egt_amd import _lib as L
    d = ST.desc(ROWS[0])
    assert egt_lib.egt_stack_tail_form(C.byref(d), 0) is None and egt_lib.egt_stack_tail_form(C.byref(d), ST.MAX_LAYERS + 1) is None
    assert egt_lib.egt_stack_tail_form(None, 3) is None
    assert egt_lib.egt_stack_tail_form(C.byref(d), ST.MAX_LAYERS) is not None
    d.De = 24                                                   # no pair kernel of that edge width
    assert egt_lib.egt_stack_tail_form(C.byref(d), 3) is None
    d = ST.desc(ROWS[0])
    d.flags |= L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN               # egt_stack_* refuses the static-edge mode
    assert egt_lib.egt_stack_tail_form(C.byref(d), 3) is None


def test_sum_class_boundaries():
    want = {1: "idle", 7: "idle", 8: "partial", 56: "partial", 57: "mixed", 63: "mixed", 64: "full", 65: "full+partial",
            128: "full", 144: "full+partial", 384: "full", 512: "full"}
    assert {n: ST.sum_class(n) for n in want} == want


def test_the_table_covers_the_launch_plane():
    ps = {row: ST.plan_tail(*row) for row in ROWS}
    classes = {p["edge_class"] for p in ps.values()} | {p["weight_class"] for p in ps.values()}
    assert classes == {"idle", "partial", "mixed", "full", "full+partial"}
    assert {"mixed", "full", "full+partial"} <= {p["edge_class"] for p in ps.values()}
    long_walk = [p for p in ps.values() if p["rows_per_wg"] > ST.WG_ROWS]
    assert {5, 6} <= {p["steps"] for p in long_walk}
    assert any(p["last_step_rows"] < ST.STEP for p in long_walk)
    assert any(p["last_step_rows"] < ST.STEP and not p["d64"] for p in long_walk)
    assert any(p["last_chunk_rows"] < p["rows_per_wg"] - ST.STEP for p in long_walk), "a last chunk that ends steps early"
    lys = {row[4] for row in ROWS}
    assert {ST.SUM_LAYERS, ST.SUM_LAYERS + 1, ST.EPG_LAYERS, ST.PRE_STACK[1], ST.MAX_LAYERS} <= lys
    assert any(ST.PRE_STACK[1] < ly < ST.MAX_LAYERS for ly in lys)
    assert {p["prep"] for p in ps.values()} == {"stack16", "stack40", "edge_prep"}
    assert {p["bwd"] for p in ps.values()} == {"k_narrow_bwd", "k_block_bwd_v4r", "k_block_bwd_v5"}
    # what the older stack parity shapes reach of it: 128 rows per workgroup, at most three chunks, no full round alone
    old = [ST.plan_tail(*row) for row in ST.EXISTING]
    assert all(p["rows_per_wg"] == ST.WG_ROWS and p["chunks"] <= 3 for p in old)
    assert not {"mixed", "full"} & {p["edge_class"] for p in old}


def test_memcontract_rows_are_rows_of_the_table(egt_lib):
    assert len(M.STACK_TAIL_TABLE) == len(ST.MEMCONTRACT_ROWS)
    for (mrow, layers), row in zip(M.STACK_TAIL_TABLE, ST.MEMCONTRACT_ROWS):
        _, B, N, d, De, bf16, extras, fwd, bwd = mrow
        assert (B, N, De, 8 * d, layers) == row and not bf16 and extras == ""
        # the training flag of the memory-contract descriptor does not move the plan: same forms, same tail
        desc = M.block_desc(mrow)
        assert egt_lib.egt_block_launch_form(C.byref(desc)).decode() == f"fwd={fwd} bwd={bwd}"
        assert bwd == ST.plan_tail(*row)["bwd_form"]
        assert egt_lib.egt_stack_tail_form(C.byref(desc), layers).decode() == ST.plan_tail(*row)["tail_form"]


@pytest.mark.parametrize("row", ROWS, ids=ST.row_id)
def test_fp32_oracle_is_within_the_fairness_cap(row):
    """FAIRNESS (tests/conditioning.py): the same oracle code in fp32 on the CPU stays within CAP = 0.25 of the tolerances of
    tests/test_stack_tail_gpu.py, so a kernel that fails there is at least four times worse than plain fp32 arithmetic.
    Worst margins of this recipe: 0.035 / 0.010 / 0.027 / 0.007 on the four large rows (in the table's order), 0.007 / 0.007 /
    0.008 on the small ones."""
    m = ST.margins(ST.run_oracle(row, torch.float32), ST.oracle(row))
    assert len(m) == 4 + 14 * row[4]
    worst = max(m, key=m.get)
    print(f"{ST.row_id(row)}: fp32 oracle worst margin {m[worst]:.4f} ({worst})")
    assert m[worst] <= ST.CAP, f"{ST.row_id(row)}: {worst} at {m[worst]:.3f} of the tolerance in plain fp32"
    inp = ST.make_inputs(row)
    n = inp["mask"].sum(1)
    assert int(n[0]) == row[1] and row[1] // 2 <= int(n.min()) < row[1], "the padding recipe"
