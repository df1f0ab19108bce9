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


# ---------------------------------------------------------------------------------- shifted arenas and the U runs -----
@pytest.mark.parametrize("shift", [4, 8, 12, 508])
@pytest.mark.parametrize("nbytes", [4, 100, 4 * 8 * 24])
def test_shifted_arena_layout(nbytes, shift):
    a, ref = M.Arena("buf", nbytes, "cpu", shift=shift), M.Arena("buf", nbytes, "cpu")
    assert a.payload.numel() == nbytes                                   # still exact
    assert a.payload.data_ptr() % 512 == shift
    assert a.before.numel() == ref.before.numel() + shift and a.after.numel() == ref.after.numel()
    assert a.before.data_ptr() % 512 == 0
    assert a.before.data_ptr() + a.before.numel() == a.payload.data_ptr()      # guards directly adjacent on both sides
    assert a.after.data_ptr() == a.payload.data_ptr() + nbytes
    assert a.view(torch.float32, (nbytes // 4,)).data_ptr() == a.payload.data_ptr()
    a.check()
    for side, idx, where in (("before", a.offset - 1, (1, 1)), ("after", a.offset + nbytes, (0, 0))):
        a.buf[idx] ^= 0x01
        assert a.guard_faults() == [(side, *where)]
        with pytest.raises(M.GuardError, match=f"guard {side} the payload"):
            a.check()
        a.buf[idx] ^= 0x01
    a.check()


def _down16(t):
    """the tensor's elements as seen through its pointer rounded down to 16 bytes (what a vector access at an address it
    took for aligned does)"""
    return t.as_strided(t.shape, t.stride(), t.storage_offset() - (t.data_ptr() % 16) // t.element_size())


def _toy_param(sink_down16=False, param_down16=False, sink_overrun=False):
    """g = 3 w, y = x + w[0]: a 'kernel' with one parameter and one gradient sink, with switchable alignment bugs"""
    w, x = torch.arange(1, 9, dtype=torch.float32) / 8, torch.arange(8, dtype=torch.float32)

    def step(v):
        wv = _down16(v["w"]) if param_down16 else v["w"]
        gv = _down16(v["g"]) if sink_down16 else v["g"]
        gv[:] = 3.0 * wv
        if sink_overrun and v["g"].data_ptr() % 16:      # a 16-byte store that starts inside the sink and ends past it
            v["g"].as_strided((4,), (1,), v["g"].storage_offset() + 8 - (v["g"].data_ptr() % 16) // 4)[:] = 3.0 * wv[4:]
        v["y"][:] = v["x"] + wv[0]
        return 0
    return M.Case("toyp", [M.Buf("x", M.IN, x), M.Buf("w", M.IN, w, ptr=M.PARAM), M.Buf("y", M.OUT, dtype=torch.float32, shape=(8,)),
                           M.Buf("g", M.OUT, dtype=torch.float32, shape=(8,), ptr=M.SINK)], [step])


def test_shift_assignment():
    case = _toy_param()
    assert [b.name for b in M.tagged(case)] == ["w", "g"]
    assert M.shifts(case, "sinks") == {"g": 8} and M.shifts(case, "all") == {"w": 4, "g": 8} == M.shifts(case, "mixed")
    bufs = [M.Buf("a", M.IN, torch.zeros(3))]
    for i in range(8):
        bufs += [M.Buf(f"p{i}", M.IN, torch.zeros(2), ptr=M.PARAM), M.Buf(f"g{i}", M.OUT, dtype=torch.float32, shape=(2,), ptr=M.SINK)]
    case = M.Case("many", bufs, [])
    al = M.shifts(case, "all")
    assert list(al) == [b.name for b in bufs[1:]] and list(al.values()) == [4 * (1 + i % 3) for i in range(16)]
    assert M.shifts(case, "sinks") == {k: v for k, v in al.items() if k[0] == "g"}
    mixed = M.shifts(case, "mixed")
    assert set(mixed) == {f"{c}{j}" for c in "pg" for j in (0, 3, 4, 7)} and all(al[k] == v for k, v in mixed.items())
    with pytest.raises(AssertionError):                                  # an activation cannot be a sink, an output no parameter
        M.Buf("x", M.OUT, dtype=torch.float32, shape=(2,), ptr=M.PARAM)


def test_u_runs_pass_a_clean_kernel_and_catch_alignment_bugs():
    z = M.check(_toy_param(), "cpu")
    assert torch.equal(z["g"], 3.0 * torch.arange(1, 9, dtype=torch.float32) / 8)
    with pytest.raises(M.GuardError, match=r"'toyp:g'.*guard before the payload.*shifted \{'g': 8\}"):     # U-sinks
        M.check(_toy_param(sink_down16=True), "cpu")
    with pytest.raises(M.GuardError, match=r"'toyp:g'.*guard after the payload.*bytes 0\.\.7 past its end"):
        M.check(_toy_param(sink_overrun=True), "cpu")
    with pytest.raises(AssertionError, match="run U-all differs from run Z") as ei:       # U-sinks passed: the parameter was aligned there
        M.check(_toy_param(param_down16=True), "cpu")
    assert not isinstance(ei.value, M.GuardError)
    M.check(_toy_param(param_down16=True), "cpu", u_runs=("sinks",))
    M.check(_toy_param(sink_down16=True, param_down16=True), "cpu", u_runs=())            # (and Z, P alone see neither)


def test_cases_without_a_pointer_class_run_as_before():
    seen = []
    case = _toy()
    step = case.steps[0]
    case.steps[0] = lambda v: (seen.append(1), step(v))[1]
    M.check(case, "cpu")
    assert len(seen) == 3                                                # Z, P, one A


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


def _param_slots(case):
    """non-NULL parameter slots of the case's call, from the ABI's own field lists"""
    from egt_amd import _lib as L
    n = case.name
    if "row" in case.claims:
        return case.claims["layers"] * (len(L.BLOCK_PARAM_FIELDS) - (len(M.STATIC_NULL) if "static" in case.claims["row"][6] else 0))
    if n.startswith("pair_"):
        return len(M.PAIR_SLOTS)
    if n.startswith("edge_proj"):
        return 2 + 2 * ("_ln" in n) + 2 * ("_gates" in n)
    if n.startswith("edge_update"):
        return 2
    if n.startswith("ffn_"):
        return len(L.FFN_PARAM_FIELDS)
    if n.startswith("embed"):
        return 3 + ("_vn" in n)
    if n.startswith("edge_head"):
        return len(L.HEAD_PARAM_FIELDS)
    if n.startswith("node_head"):
        return len(L.NODE_HEAD_PARAM_FIELDS)
    if n.startswith("distance_target"):
        return 0
    raise AssertionError(n)


@pytest.mark.parametrize("family", ["block", "stack", "pair", "edge", "ffn", "embed", "head"])
def test_parameters_and_sinks_of_the_table_are_tagged(family, egt_lib):
    cases = M.FAMILIES[family](egt_lib)
    assert cases
    for case in cases:
        slots = _param_slots(case)
        assert slots or case.name.startswith("distance_target")          # (the one entry point of these families without parameters)
        tg = M.tagged(case)
        params, sinks = [b for b in tg if b.ptr == M.PARAM], [b for b in tg if b.ptr == M.SINK]
        assert len(params) == len(sinks) == slots, f"{case.name}: {len(params)} parameters, {len(sinks)} sinks, {slots} slots"
        assert sorted(b.shape for b in params) == sorted(b.shape for b in sinks)
        assert all(b.dtype == torch.float32 for b in tg)
        for b in case.bufs:                                              # nothing else: workspaces, saved buffers, activations
            if b.role in (M.CARRIED, M.SCRATCH, M.INOUT) or b.dtype != torch.float32:
                assert b.ptr is None, f"{case.name}:{b.name}"
        if len(tg) >= 3:
            assert set(M.shifts(case, "all").values()) == {4, 8, 12}, case.name
        sh = M.shifts(case, "sinks")                                     # neighbouring sinks differ in the sinks-only run too
        assert len(sh) < 2 or len(set(sh.values())) >= 2, case.name
        if slots:
            sh = M.shifts(case, "mixed")
            assert 0 < len(sh) < len(tg) and set(M.shifts(case, "sinks")) == {b.name for b in sinks}
            for cls in (params, sinks):                                  # aligned and unaligned pointers of both classes in one call
                assert 0 < sum(b.name in sh for b in cls) < len(cls) or len(cls) < 2
    if family in ("block", "stack"):            # the two weights the node kernels test separately sit on different sides
        for case in cases:
            sh = M.shifts(case, "mixed")
            for l in range(case.claims["layers"]):
                assert (f"p{l}.dense_qkv_kernel" in sh) != (f"p{l}.dense_mha_kernel" in sh), case.name


@pytest.mark.parametrize("family", ["attn", "mfma", "mask"])
def test_families_without_parameters_have_no_tagged_buffer(family, egt_lib):
    assert all(not M.tagged(c) for c in M.FAMILIES[family](egt_lib))
