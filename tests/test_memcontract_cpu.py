"""tests/memcontract.py without a GPU: the harness must be able to fail (a checker that cannot fail proves nothing), and the
block / stack case table must reach the kernels it claims (egt_block_launch_form answers without a GPU: egt_device_cus() falls
back to 256).  A later change of a plan rule that silently moves a case onto another kernel fails here."""
import ctypes as C

import pytest
import torch

import memcontract as M


# --------------------------------------------------------------------------------------------- harness self-test -----
@pytest.mark.parametrize("nbytes,graphs", [(1, 1), (100, 1), (4 * 19 * 19 * 8 * 2, 2), (3 * 1000003, 3)])
def test_arena_layout(nbytes, graphs):
    a = M.Arena("buf", nbytes, "cpu", graphs)
    assert a.payload.numel() == nbytes                                   # exact: no rounding up
    assert a.payload.data_ptr() % 512 == 0 and a.offset % 512 == 0       # 512-aligned payload
    assert a.before.numel() == a.after.numel() >= max(4096, -(-nbytes // graphs))
    assert a.before.numel() % 512 == 0
    assert a.before.data_ptr() + a.before.numel() == a.payload.data_ptr()
    assert a.after.data_ptr() == a.payload.data_ptr() + nbytes
    assert a.guard_faults() == []
    a.check()


def test_guards_are_a_seeded_pattern():
    a, b, c = M.Arena("x", 64), M.Arena("x", 64), M.Arena("y", 64)
    assert torch.equal(a.before, b.before) and torch.equal(a.after, b.after)
    assert not torch.equal(a.before, c.before)
    assert len(torch.unique(a.before)) > 100            # not a constant fill: a kernel that writes zeros or 0xFF cannot blend in


def test_payload_views_alias_the_arena():
    a = M.Arena("v", 4 * 6, "cpu")
    v = a.view(torch.float32, (2, 3))
    assert v.data_ptr() == a.payload.data_ptr()
    v.fill_(1.0)
    assert torch.equal(a.payload.view(torch.float32), torch.ones(6))
    a.check()                                            # a write inside the payload is not reported
    a.payload[0] ^= 0xFF
    a.payload[-1] ^= 0xFF
    a.check()


@pytest.mark.parametrize("side", ["before", "after"])
def test_one_byte_outside_the_payload_is_reported(side):
    a = M.Arena("case:d_e", 1000, "cpu")
    if side == "before":
        a.buf[a.offset - 1] ^= 0x01
    else:
        a.buf[a.offset + 1000] ^= 0x01
    assert a.guard_faults() == [(side, 1, 1) if side == "before" else (side, 0, 0)]
    with pytest.raises(M.GuardError) as ei:
        a.check(" by step 1")
    msg = str(ei.value)
    assert "'case:d_e'" in msg and f"guard {side} the payload" in msg and "by step 1" in msg
    assert ("1..1 before its start" if side == "before" else "0..0 past its end") in msg


def test_first_and_last_changed_offsets():
    a = M.Arena("w", 256, "cpu")
    a.after[3] ^= 1
    a.after[700] ^= 1
    a.before[-8] ^= 1
    assert a.guard_faults() == [("before", 8, 8), ("after", 3, 700)]


def _toy(overrun=0, stale=False, touch_input=False, alias_bug=False):
    """y = 2 x through a scratch word, as a 'kernel' on host tensors, with switchable contract violations"""
    x = torch.arange(1, 9, dtype=torch.float32)

    def step(v):
        n = 8 + overrun
        raw = v["y"].as_strided((n,), (1,))              # (a view past the payload: what an off-by-one store does)
        src = v["x"].clone() if alias_bug and v["y"].data_ptr() == v["x"].data_ptr() else v["x"]
        if not stale:
            v["ws"][0] = 2.0
        raw[:8] = src * v["ws"][0] + (1.0 if src is not v["x"] else 0.0)
        if overrun:
            raw[8:] = 7.0
        if touch_input:
            v["x"][2] = 0.0
        return 0
    return M.Case("toy", [M.Buf("x", M.IN, x), M.Buf("y", M.OUT, dtype=torch.float32, shape=(8,)),
                          M.Buf("ws", M.SCRATCH, nbytes=4, dtype=torch.float32, shape=(1,))], [step], [{"y": "x"}])


def test_runner_passes_a_clean_case_and_catches_each_violation():
    z = M.check(_toy(), "cpu")
    assert torch.equal(z["y"], 2.0 * torch.arange(1, 9, dtype=torch.float32))
    with pytest.raises(M.GuardError, match="'toy:y'.*guard after"):
        M.check(_toy(overrun=1), "cpu")
    with pytest.raises(AssertionError, match="not finite"):                      # scratch read before it was written
        M.check(_toy(stale=True), "cpu")
    with pytest.raises(AssertionError, match="const buffer 'toy:x'"):
        M.check(_toy(touch_input=True), "cpu")
    with pytest.raises(AssertionError, match="differs from run Z"):             # result depends on the aliasing
        M.check(_toy(alias_bug=True), "cpu")


def test_read_modify_write_exception_covers_only_its_elements():
    """a CARRIED buffer that is const from step 0 on, except the elements its rmw entry names (rowstats slot 3)"""
    def case(slot):
        def fwd(v):
            v["stats"][:] = torch.arange(8, dtype=torch.float32).view(2, 4)
            return 0

        def bwd(v):
            v["stats"][:, slot] = 9.0
            return 0
        return M.Case("rmw", [M.Buf("stats", M.CARRIED, dtype=torch.float32, shape=(2, 4), compare=True, const_after=0,
                                    rmw={1: ("slot 3 written", lambda t: torch.arange(4) == 3)})], [fwd, bwd])
    M.check(case(3), "cpu")
    with pytest.raises(AssertionError, match="const buffer 'rmw:stats' was written by step 1.*2 elements"):
        M.check(case(0), "cpu")


def test_prefill_dependence_without_nan_is_caught():
    def step(v):
        v["y"][:4] = 1         # the upper half is never written
        return 0
    case = M.Case("half", [M.Buf("y", M.OUT, dtype=torch.uint8, shape=(8,))], [step])
    with pytest.raises(AssertionError, match="'half:y': run P differs from run Z in 4/8"):
        M.check(case, "cpu")
    case.bufs[0].exempt = ("a sentence of the header", lambda t: torch.arange(8) >= 4)
    M.check(case, "cpu")


# ------------------------------------------------------------------------------------------------- the case table -----
def _forms(lib, desc):
    s = lib.egt_block_launch_form(C.byref(desc))
    assert s is not None
    fwd, bwd = s.decode().split()
    return fwd[len("fwd="):], bwd[len("bwd="):]


@pytest.mark.parametrize("row", M.BLOCK_TABLE + M.STACK_TABLE, ids=lambda r: r[0])
def test_table_reaches_the_kernels_it_claims(row, egt_lib):
    desc = M.block_desc(row)
    assert egt_lib.egt_block_supported(C.byref(desc)) == 1
    fwd, bwd = _forms(egt_lib, desc)
    assert (fwd, bwd) == (row[7], row[8])
    assert egt_lib.egt_block_bwd_kernel(C.byref(desc)).decode() == row[8].split("/")[0]


def test_table_covers_every_family_and_wave_count():
    fwd = {r[7] for r in M.BLOCK_TABLE + M.STACK_TABLE}
    bwd = {r[8] for r in M.BLOCK_TABLE + M.STACK_TABLE}
    reach_f = fwd | {f.split("/")[0] for f in fwd if f.startswith("k_block_fwd/")}
    reach_b = {"/".join(b.split("/")[:2]) for b in bwd if b.startswith("k_narrow")} | {b.split("/")[0] for b in bwd}
    assert M.REQUIRED_FORMS["fwd"] <= reach_f, M.REQUIRED_FORMS["fwd"] - reach_f
    assert M.REQUIRED_FORMS["bwd"] <= reach_b, M.REQUIRED_FORMS["bwd"] - reach_b
    assert {"static", "attn_mask", "rand_mask"} <= {x for r in M.BLOCK_TABLE for x in r[6].split(",")}
    assert any(r[5] for r in M.BLOCK_TABLE) and any(r[5] for r in M.STACK_TABLE)         # bf16 edge tensors in both


def test_every_size_query_of_the_table_is_non_zero(egt_lib):
    n = 0
    for case in M.all_cases(egt_lib):
        for b in case.bufs:
            if b.role in (M.CARRIED, M.SCRATCH):
                assert b.nbytes > 0, f"{case.name}: size query of '{b.name}' answers 0"
                n += 1
        assert case.steps
    assert n > 100
