"""Attention dropout on the fused block, pinned without a GPU (library built): the library's answers, flag checks, launch forms and
sizes for descriptors with EGT_BF_ATTN_DROPOUT; the route table of egt_amd.fused.route_core with and without the opt-in
(EGTBlock(fused_attn_dropout=True)); the seeds a flagged call consumes; the config key; and the fp64 oracle against the reference
fixtures of tests/golden/attn_dropout/."""
import ctypes as C
import os

import pytest
import torch

import attn_dropout_cases as AC
from oracle import ref_exec as RX
from test_fused_host_cpu import (_call, _desc, ENTRIES, RES, BIAS, COMPOSED, NARROW, EDGE_DTYPE, ROUTE_CASES, _case, make_block, PTR)


def _do(L, De=64, flags=0, rate=0.25, dtype=None, N=19, d=8, B=2, prob=0.0, training=True):
    """a descriptor flagged EGT_BF_ATTN_DROPOUT (with EGT_BF_TRAINING unless told otherwise), the rate in `reserved`"""
    desc = _desc(L, De=De, flags=L.BF_ATTN_DROPOUT | (L.BF_TRAINING if training else 0) | flags, prob=prob)
    desc.N, desc.d, desc.B = N, d, B
    desc.reserved = L.rate_bits(rate)
    if dtype is not None:
        desc.dtype = dtype
    return desc


# ----------------------------------------------------------------------------------------- the library's answers -----
def test_rate_bits_round_trip():
    import struct
    from egt_amd import _lib as L
    for r in (0.1, 0.25, 0.5):
        assert struct.unpack("<f", struct.pack("<i", L.rate_bits(r)))[0] == struct.unpack("<f", struct.pack("<f", r))[0]
    assert L.rate_bits(0.0) == 0


def test_flag_header_and_ctypes_agree():
    """the new bit is the next one after EGT_BF_SCALER_LINEAR, mirrors the header, and no struct changed its layout (ABI 4)"""
    import re
    from egt_amd import _lib as L
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egt_amd.h")).read()
    assert re.search(r"#define EGT_BF_ATTN_DROPOUT \(EGT_BF_SCALER_LINEAR << 1\)", src)
    assert L.BF_ATTN_DROPOUT == L.BF_SCALER_LINEAR << 1 == 0x200
    others = (L.BF_GATE | L.BF_ATTN_MASK | L.BF_TRAINING | L.BF_CLIP | L.BF_NO_EDGE_LN | L.BF_SEED_DEVICE | L.BF_STATIC_EDGE
              | L.BF_SCALE_DEGREE | L.BF_SCALER_LINEAR)
    assert not (others & L.BF_ATTN_DROPOUT)
    assert re.search(r"#define EGT_ABI_VERSION (\d+)", src).group(1) == str(L.ABI_VERSION) == "4"
    assert [f for f, _ in L.BlockDesc._fields_].count("reserved") == 1          # the rate's four bytes keep their name


@pytest.mark.parametrize("row", list(AC.SHAPES) + list(AC.VARIANTS))
def test_library_covers_the_table(egt_lib, row):
    """every row of the GPU table: covered, its launch form names the families the table names, sizes equal the unflagged descriptor's"""
    from egt_amd import _lib as L
    v = AC.VARIANTS.get(row, dict(shape=row))
    B, N, d, De, _, ffwd, fbwd = AC.SHAPES[v["shape"]]
    ffwd, fbwd = v.get("fwd", ffwd), v.get("bwd", fbwd)
    extra = 0
    if v.get("ect") == "constrained":
        extra |= L.BF_ATTN_MASK
    if v.get("ect") == "bias":
        extra |= L.BF_NO_EDGE_LN
    for rate, prob in AC.RATES.values():
        flagged = _do(L, De=De, flags=extra, rate=rate, N=N, d=d, B=B, prob=prob)
        if v.get("gate") is False:
            flagged.flags &= ~L.BF_GATE
        plain = _do(L, De=De, flags=extra, rate=rate, N=N, d=d, B=B, prob=prob)
        plain.flags = flagged.flags & ~L.BF_ATTN_DROPOUT
        plain.reserved = 0
        assert egt_lib.egt_block_supported(C.byref(flagged)) == 1
        assert egt_lib.egt_pair_supported(C.byref(flagged)) == 0
        form = egt_lib.egt_block_launch_form(C.byref(flagged)).decode()
        assert f"fwd={ffwd}" in form and f"bwd={fbwd}/" in form, (row, form)
        assert egt_lib.egt_block_bwd_kernel(C.byref(flagged)).decode() == fbwd
        assert egt_lib.egt_block_saved_bytes(C.byref(flagged)) == egt_lib.egt_block_saved_bytes(C.byref(plain)) > 0
        assert egt_lib.egt_block_workspace_bytes(C.byref(flagged)) == egt_lib.egt_block_workspace_bytes(C.byref(plain)) > 0
        if De != 8:          # same families as the unflagged plan; De = 8 leaves the VALU kernels (next test)
            assert egt_lib.egt_block_launch_form(C.byref(plain)).decode() == form


@pytest.mark.parametrize("row,fwd,bwd", [(r, *f) for r, f in AC.BF16_ROWS.items()])
def test_bf16_rows(egt_lib, row, fwd, bwd):
    from egt_amd import _lib as L
    B, N, d, De, _, _, _ = AC.SHAPES[row]
    desc = _do(L, De=De, N=N, d=d, B=B, dtype=L.EGT_BF16)
    assert egt_lib.egt_block_supported(C.byref(desc)) == 1
    form = egt_lib.egt_block_launch_form(C.byref(desc)).decode()
    assert f"fwd={fwd}" in form and f"bwd={bwd}/" in form, form


@pytest.mark.parametrize("N,B", [(19, 2), (69, 2), (150, 2), (120, 16)])
@pytest.mark.parametrize("bf16", [False, True])
def test_de8_runs_on_the_mfma_tile_kernels(egt_lib, N, B, bf16):
    """with the flag De = 8 takes k_block_fwd_r4 / k_block_bwd_v4r (egt_narrow.hip draws no dropout), as under EGT_NO_NARROW=1"""
    from egt_amd import _lib as L
    d = _do(L, De=8, N=N, B=B, dtype=L.EGT_BF16 if bf16 else None)
    form = egt_lib.egt_block_launch_form(C.byref(d)).decode()
    assert form.startswith("fwd=k_block_fwd_r4/") and " bwd=k_block_bwd_v4r/4w/" in form, form
    plain = _desc(L, De=8); plain.N, plain.B = N, B
    assert "k_narrow" in egt_lib.egt_block_launch_form(C.byref(plain)).decode()      # (the unflagged plan is untouched)
    assert egt_lib.egt_block_saved_bytes(C.byref(d)) > 0 and egt_lib.egt_block_workspace_bytes(C.byref(d)) > 0


def test_every_edge_width_and_flag_mix(egt_lib):
    from egt_amd import _lib as L
    for De in (8, 16, 32, 48, 64):
        for dtype in (L.EGT_F32, L.EGT_BF16):
            for extra in (0, L.BF_ATTN_MASK, L.BF_NO_EDGE_LN, L.BF_SEED_DEVICE):
                d = _do(L, De=De, flags=extra, dtype=dtype)
                if extra == L.BF_SEED_DEVICE:
                    d.seed_device = PTR
                assert egt_lib.egt_block_supported(C.byref(d)) == 1, (De, dtype, extra)
            ungated = _do(L, De=De, dtype=dtype); ungated.flags &= ~L.BF_GATE
            assert egt_lib.egt_block_supported(C.byref(ungated)) == 1
    # the refusals, as answers
    assert egt_lib.egt_block_supported(C.byref(_do(L, training=False))) == 0
    assert egt_lib.egt_block_supported(C.byref(_do(L, flags=L.BF_SCALE_DEGREE))) == 0
    assert egt_lib.egt_block_supported(C.byref(_do(L, De=8, flags=L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN))) == 0
    for rate in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert egt_lib.egt_block_supported(C.byref(_do(L, rate=rate))) == 0, rate
    # without the flag `reserved` is ignored, as before
    junk = _desc(L); junk.reserved = L.rate_bits(7.0)
    assert egt_lib.egt_block_supported(C.byref(junk)) == 1
    # the pair operator's own geometry (d = 64, De = 32): covered without the flag, not with it
    plain = _desc(L, De=32); plain.d, plain.N = 64, 16
    assert egt_lib.egt_pair_supported(C.byref(plain)) == 1 and egt_lib.egt_pair_block_supported(C.byref(plain)) == 1
    flagged = _do(L, De=32, d=64, N=16)
    assert egt_lib.egt_pair_supported(C.byref(flagged)) == 0 and egt_lib.egt_pair_block_supported(C.byref(flagged)) == 0
    assert egt_lib.egt_block_supported(C.byref(flagged)) == 0
    assert egt_lib.egt_pair_block_saved_bytes(C.byref(flagged)) == 0 and egt_lib.egt_pair_block_workspace_bytes(C.byref(flagged)) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_flag_rules(egt_lib, entry):
    """every refusal by code and message, answered before any launch (dummy pointers)"""
    from egt_amd import _lib as L
    stack = entry.startswith("egt_stack")

    def expect(code, text, desc, **kw):
        rc, msg = _call(egt_lib, L, entry, desc, **kw)
        assert rc == code and text in msg, (entry, rc, msg)

    if stack:      # refused like EGT_BF_SCALE_DEGREE, flags before pointers and sizes
        expect(L.EGT_E_FLAGS, "egt_stack_* does not take EGT_BF_ATTN_DROPOUT", _do(L))
        expect(L.EGT_E_FLAGS, "egt_stack_* does not take EGT_BF_ATTN_DROPOUT", _do(L), h=None)
        d = _do(L)
        assert egt_lib.egt_stack_saved_bytes(C.byref(d), 2) == 0 and egt_lib.egt_stack_workspace_bytes(C.byref(d), 2) == 0
        return
    expect(L.EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT needs EGT_BF_TRAINING", _do(L, training=False))
    expect(L.EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT does not take EGT_BF_SCALE_DEGREE", _do(L, flags=L.BF_SCALE_DEGREE))
    expect(L.EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT does not take EGT_BF_STATIC_EDGE", _do(L, De=8, flags=L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN))
    for rate, shown in ((0.0, "got 0"), (1.0, "got 1"), (1.5, "got 1.5"), (-0.25, "got -0.25")):
        rc, msg = _call(egt_lib, L, entry, _do(L, rate=rate))
        assert rc == L.EGT_E_FLAGS and "EGT_BF_ATTN_DROPOUT needs a rate in (0, 1)" in msg and shown in msg, (rate, rc, msg)
    d = _do(L)
    for q in ("egt_block_saved_bytes", "egt_block_workspace_bytes"):
        assert getattr(egt_lib, q)(C.byref(_do(L, training=False))) == 0 and getattr(egt_lib, q)(C.byref(d)) > 0
    assert egt_lib.egt_block_launch_form(C.byref(_do(L, rate=1.0))) is None
    # a flagged, valid descriptor passes the flag checks: the next complaint is about the pointers
    expect(L.EGT_E_NULL, "is NULL", _do(L), h=None)


# ------------------------------------------------------------------------------------------------- route table -----
OPT = dict(attn_dropout=0.1, fused_attn_dropout=True)
OPT_CASES = [
    _case("do_De64", RES, **OPT),
    _case("do_d6_De48", RES, model_width=48, edge_width=48, **OPT),
    _case("do_De8", RES, **OPT, **NARROW),
    _case("do_De8_bf16", RES, edge="bf16", **OPT, **NARROW),
    _case("do_De64_bf16", RES, edge="bf16", **OPT),
    _case("do_train", RES, train=True, **OPT),
    _case("do_train_in_kernel_mask", RES, train=True, random_mask_prob=0.1, **OPT),
    _case("do_train_host_rand_mask", RES, train=True, rand_mask=True, random_mask_prob=0.1, **OPT),
    _case("do_constrained_mask", RES, attn_mask=True, edge_channel_type="constrained", **OPT),
    _case("do_constrained_no_mask", COMPOSED, edge_channel_type="constrained", **OPT),
    _case("do_ungated", RES, gate_attention=False, **OPT),
    _case("do_bias_alone_De8", BIAS, edge_channel_type="bias", **OPT, **NARROW),
    _case("do_bias_in_stack_De8", BIAS, in_stack=True, edge_channel_type="bias", **OPT, **NARROW),      # never "static"
    _case("do_bias_De64", BIAS, edge_channel_type="bias", **OPT),
    _case("do_scale_degree", COMPOSED, scale_degree=True, **OPT),
    _case("do_virtual_nodes", COMPOSED, num_virtual_nodes=1, **OPT),
    _case("do_node_dropout_train", COMPOSED, train=True, node_dropout=0.1, **OPT),
    _case("do_width512_pair_geometry", COMPOSED, N=16, model_width=512, edge_width=32, **OPT),
    _case("do_fused_off", COMPOSED, fused="off", **OPT),
    _case("do_scale_degree_fused_true", RuntimeError, scale_degree=True, fused=True, **OPT),
    _case("opt_in_without_a_rate", RES, fused_attn_dropout=True),                                        # nothing to draw: as today
    _case("rate_without_opt_in", COMPOSED, attn_dropout=0.1),
    _case("rate_without_opt_in_bf16", COMPOSED, edge="bf16", attn_dropout=0.1),
]


def _route(case, **over):
    from egt_amd import fused as FZ
    blk = make_block(case)
    args = (blk, 2, case["N"], torch.float32, EDGE_DTYPE[case["edge"]], True)
    kw = dict(attn_mask=case["attn_mask"], rand_mask=case["rand_mask"], training=case["train"])
    kw.update(over)
    return FZ.route_core(*args, **kw)


@pytest.mark.parametrize("case", OPT_CASES, ids=lambda c: c["name"])
def test_route_table_with_the_opt_in(egt_lib, case):
    from egt_amd import fused as FZ
    old, FZ._NO_STATIC_EDGE = FZ._NO_STATIC_EDGE, False
    try:
        if case["want"] is RuntimeError:
            with pytest.raises(RuntimeError, match="not covered"):
                _route(case)
            return
        assert _route(case) == case["want"]
        if case["want"][0] == "fused" and not case["train"]:      # training and evaluation: the same route
            assert _route(case, training=True) == case["want"]
    finally:
        FZ._NO_STATIC_EDGE = old


@pytest.mark.parametrize("case", [c for c in ROUTE_CASES if "fused_attn_dropout" not in c["kw"]], ids=lambda c: c["name"])
def test_rows_without_the_opt_in_answer_as_before(egt_lib, case):
    """tests/test_fused_host_cpu.py's table with fused_attn_dropout=False spelled out: every answer is ROUTE_CASES' own"""
    from egt_amd import fused as FZ
    c = dict(case, kw=dict(case["kw"], fused_attn_dropout=False))
    old, FZ._NO_STATIC_EDGE = FZ._NO_STATIC_EDGE, bool(case["no_static"])
    try:
        if case["want"] is RuntimeError:
            with pytest.raises(RuntimeError, match="not covered"):
                _route(c)
        else:
            assert _route(c) == case["want"]
    finally:
        FZ._NO_STATIC_EDGE = old


def test_unsupported_messages(egt_lib):
    from egt_amd import fused as FZ
    from egt_amd.layers import EGTBlock
    mk = lambda **kw: EGTBlock(model_width=64, edge_width=64, **kw)
    assert FZ._unsupported(mk(attn_dropout=0.1), True) == "scale_degree / attn_dropout / virtual nodes"          # as today
    assert FZ._unsupported(mk(attn_dropout=0.1, fused_attn_dropout=False), False) == "scale_degree / attn_dropout / virtual nodes"
    assert FZ._unsupported(mk(**OPT), True) is None and FZ._unsupported(mk(**OPT), False) is None
    why = FZ._unsupported(mk(scale_degree=True, **OPT), True)
    assert "attn_dropout" in why and "scale_degree" in why and why != "scale_degree / attn_dropout / virtual nodes"
    assert FZ._unsupported(mk(num_virtual_nodes=1, **OPT), True) == "scale_degree / attn_dropout / virtual nodes"
    assert FZ._unsupported(mk(node_dropout=0.1, **OPT), True) == "node / edge dropout"
    # bf16: the refusal that existing tests match stays without the opt-in, and goes with it
    assert "attn_dropout" in FZ.bf16_refusal(mk(attn_dropout=0.1))
    assert FZ.bf16_refusal(mk(**OPT)) is None
    assert FZ.bf16_refusal(EGTBlock(model_width=64, edge_width=8, **OPT)) is None
    assert "head dim 64" in FZ.bf16_refusal(EGTBlock(model_width=512, edge_width=32, **OPT))


def test_flags_and_memo_see_the_bit(egt_lib):
    from egt_amd import fused as FZ, _lib as L
    from egt_amd.layers import EGTBlock
    blk = EGTBlock(model_width=64, edge_width=64, **OPT)
    assert FZ._flags(blk) & L.BF_ATTN_DROPOUT == 0                       # evaluation / the unflagged question
    f = FZ._flags(blk, dropout=True)
    assert f & L.BF_ATTN_DROPOUT and f & L.BF_TRAINING
    d = FZ._desc(blk, 2, 19, False, 5, dropout=True)
    assert d.reserved == L.rate_bits(0.1) and d.flags & L.BF_ATTN_DROPOUT
    assert FZ._desc(blk, 2, 19, True, 5).reserved == 0
    FZ.route_core(blk, 2, 19, torch.float32, torch.float32, True)
    keys = [k for k in FZ._LIB_ANSWERS if k[0] == "egt_block_supported" and k[2] == 19 and k[5] == 64 and k[7] & L.BF_ATTN_DROPOUT]
    assert keys and all(k[8] == L.rate_bits(0.1) for k in keys)
    n = len(FZ._LIB_ANSWERS)
    FZ.route_core(blk, 2, 19, torch.float32, torch.float32, True)
    assert len(FZ._LIB_ANSWERS) == n                                      # answered from the memo
    blk.mha.attn_dropout = 0.3                                            # another rate: another descriptor
    FZ.route_core(blk, 2, 19, torch.float32, torch.float32, True)
    assert len(FZ._LIB_ANSWERS) == n + 1


def test_stack_call_is_not_taken(egt_lib):
    """egt_stack_* refuses the flag, so an EGTStack of such blocks runs block by block (fused.stack_supported)"""
    from egt_amd import fused as FZ
    from egt_amd.layers import EGTStack
    st = EGTStack(model_height=2, model_width=64, edge_width=64, num_heads=8, **OPT)
    h = torch.zeros(2, 19, 64); e = torch.zeros(2, 19, 19, 64)
    assert FZ.stack_supported(st, h, e, None) is False


# -------------------------------------------------------------------------------------------- seed consumption -----
class _Recorder:
    """stands where _FusedBlock stands in block_fused: records the descriptor, launches nothing"""
    descs = []

    @staticmethod
    def apply(h, e, mask, attn_mask, rand_mask, desc, first, *params):
        _Recorder.descs.append((desc, rand_mask))
        return h, e


def _fused_call(blk, rand_mask=None):
    from egt_amd import fused as FZ
    h = torch.zeros(2, 19, 64); e = torch.zeros(2, 19, 19, 64)
    _Recorder.descs.clear()
    old, FZ._FusedBlock = FZ._FusedBlock, _Recorder
    try:
        FZ.block_fused(blk, h, e, None, None, rand_mask, edge_route="chained-residual")
    finally:
        FZ._FusedBlock = old
    return _Recorder.descs[-1][0]


@pytest.mark.parametrize("prob", [0.0, 0.1])
@pytest.mark.parametrize("inject", [False, True])
def test_a_flagged_call_consumes_one_seed(egt_lib, prob, inject):
    """training mode: one EGT.next_seed() per call whatever the random mask's source; the descriptor carries that seed, the flag, the rate"""
    from egt_amd import _lib as L
    from egt_amd.layers import EGTBlock
    blk = EGTBlock(model_width=64, edge_width=64, random_mask_prob=prob, seed=3, **OPT).train()
    rm = torch.zeros(2, 19, 19, 8, dtype=torch.bool) if inject else None
    for call in (1, 2):
        d = _fused_call(blk, rm)
        assert blk.mha._calls == call
        assert d.seed == AC.first_seed(3, call)
        assert d.flags & L.BF_ATTN_DROPOUT and d.flags & L.BF_TRAINING and d.reserved == L.rate_bits(0.1)
        assert d.random_mask_prob == pytest.approx(prob)
    blk.eval()                                      # evaluation: the unflagged descriptor, no seed
    d = _fused_call(blk, None)
    assert blk.mha._calls == 2 and d.seed == 0 and not d.flags & (L.BF_ATTN_DROPOUT | L.BF_TRAINING) and d.reserved == 0


@pytest.mark.parametrize("prob,inject,calls", [(0.1, False, 1), (0.1, True, 0), (0.0, False, 0)])
def test_a_block_without_the_opt_in_draws_as_before(egt_lib, prob, inject, calls):
    from egt_amd import _lib as L
    from egt_amd.layers import EGTBlock
    blk = EGTBlock(model_width=64, edge_width=64, random_mask_prob=prob, seed=3).train()
    d = _fused_call(blk, torch.zeros(2, 19, 19, 8, dtype=torch.bool) if inject else None)
    assert blk.mha._calls == calls and d.seed == (AC.first_seed(3) if calls else 0)
    assert not d.flags & L.BF_ATTN_DROPOUT and d.reserved == 0
    assert bool(d.flags & L.BF_TRAINING) == (prob > 0)


def test_device_seeds_are_used_by_a_flagged_call(egt_lib):
    """under DeviceSeeds the flagged call takes the device word (EGT_BF_SEED_DEVICE, host seed 0) and no host seed -- also with
    random_mask_prob == 0, where an unflagged block passes no seed at all"""
    from egt_amd import _lib as L
    from egt_amd.graph import DeviceSeeds
    from egt_amd.layers import EGTBlock
    blk = EGTBlock(model_width=64, edge_width=64, seed=3, **OPT).train()
    seeds = DeviceSeeds([blk.mha], "cpu")
    d = _fused_call(blk)
    assert d.flags & L.BF_SEED_DEVICE and d.seed == 0 and d.seed_device == seeds.ptr(0) and blk.mha._calls == 0
    seeds.detach()
    plain = EGTBlock(model_width=64, edge_width=64, seed=3).train()
    s2 = DeviceSeeds([plain.mha], "cpu")
    assert not _fused_call(plain).flags & L.BF_SEED_DEVICE
    s2.detach()


# --------------------------------------------------------------------------------------------------- config key -----
def test_config_key():
    from egt_amd import training as T
    c = T.make_config(dict(scheme="zinc.svd"))
    assert c.fused_attn_dropout is False
    assert "fused_attn_dropout" not in T.model_config(c)
    s = T.ZincSVDScheme(dict(scheme="zinc.svd", attn_dropout=0.1), print_fn=lambda *a: None)
    assert "fused_attn_dropout" not in s.model_kwargs() and s.model_kwargs()["attn_dropout"] == 0.1
    s = T.ZincSVDScheme(dict(scheme="zinc.svd", attn_dropout=0.1, fused_attn_dropout=True), print_fn=lambda *a: None)
    assert "fused_attn_dropout" not in s.get_model_config()                 # a project key, not a reference key
    assert s.model_kwargs()["fused_attn_dropout"] is True
    got = {}
    s.model_factory = lambda kw: got.update(kw) or "model"
    assert s.get_model() == "model" and got["fused_attn_dropout"] is True
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="fused_attn_dropout"):
            T.make_config(dict(scheme="zinc.svd", fused_attn_dropout=bad))


def test_model_keyword_reaches_every_block(egt_lib):
    from egt_amd.model import ZincDCTransformer
    kw = dict(model_width=64, edge_width=64, model_height=2, upto_hop=4, attn_dropout=0.1)
    m = ZincDCTransformer(fused_attn_dropout=True, **kw)
    assert all(b.fused_attn_dropout and b.mha.attn_dropout == 0.1 for b in m.layers.blocks)
    assert not any(b.fused_attn_dropout for b in ZincDCTransformer(**kw).layers.blocks)
    with pytest.raises(ValueError, match="fused_attn_dropout"):
        ZincDCTransformer(fused_attn_dropout="on", **kw)


@pytest.mark.parametrize("De", [64, 8])
def test_bf16_model_constructs_with_the_key_only(egt_lib, De):
    from egt_amd.model import ZincDCTransformer
    kw = dict(model_width=64, edge_width=De, model_height=2, upto_hop=4, attn_dropout=0.1, edge_dtype="bf16")
    with pytest.raises(ValueError, match="attn_dropout"):
        ZincDCTransformer(**kw)
    m = ZincDCTransformer(fused_attn_dropout=True, **kw)
    assert m.edge_dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------ reference fixtures -----
def _oracle_equals(ref, got, what):
    """to 1e-12 of each tensor's magnitude; a tensor that is zero in exact arithmetic (max |ref| < 1e-9: d(dense_edge_b.bias), a sum
    of softmax-row gradients) is rounding noise on both sides and gets the same bound as an absolute one"""
    assert set(ref) == set(got), (what, set(ref) ^ set(got))
    for k, r in ref.items():
        g = got[k].detach().double()
        assert g.shape == r.shape, (what, k)
        scale = float(r.abs().max())
        assert float((g - r).abs().max()) <= 1e-12 * (scale if scale >= 1e-9 else 1.0), (what, k, scale)


@pytest.mark.parametrize("fix", list(AC.BLOCK_FIXTURES))
def test_oracle_equals_the_reference_block_fixture(fix):
    fx = AC.load(f"{fix}.npz")
    inp, params, attrs, prob = AC.block_inputs(fix)
    for k, v in list(inp.items()) + list(params.items()):      # the stored inputs and weights ARE the seeded recipe's
        if v is not None:
            grp = "weights" if k in params else "inputs"
            assert (torch.from_numpy(fx[f"{grp}/{k}"]) == v).all(), k
    assert (inp["rand_mask"] is not None) == (prob > 0)
    keep = attrs["drop_keep"]
    assert 0.5 < float(keep.float().mean()) < 1.0                # a mask that drops something and keeps most
    _oracle_equals(AC.load_out(f"{fix}.npz"), AC.oracle_block(fix), fix)


def test_oracle_equals_the_reference_model_fixture():
    fx = AC.load("model_zinc.npz")
    inp, params, _ = AC.model_inputs()
    for k, v in inp.items():
        assert (torch.from_numpy(fx[f"inputs/{k}"]) == v).all(), k
    for k, v in params.items():
        assert (torch.from_numpy(fx[f"weights/{k}"]) == v).all(), k
    ref = AC.load_out("model_zinc.npz", "model_zinc_grads.npz")
    assert set(ref) == {"y", "loss"} | {f"d/{k}" for k in params}      # prediction, loss and EVERY weight gradient
    _oracle_equals(ref, AC.oracle_model(), "model_zinc")


@pytest.mark.skipif(not RX.available(), reason="no reference tree (EGT_REFERENCE_DIR)")
def test_the_block_fixture_is_what_the_reference_computes():
    """the committed file against a fresh run of the reference's code on the stand-in (the maker is deterministic)"""
    import numpy as np
    with RX.reference() as R:
        fresh = AC.flat(AC.ref_block(R, "block_p10_rm10"))
    stored = AC.load("block_p10_rm10.npz")
    assert set(fresh) == set(stored)
    for k, v in fresh.items():
        assert np.array_equal(np.asarray(v), stored[k]), k


def test_fixture_files_are_small_and_hold_data_only():
    import numpy as np
    names = sorted(os.listdir(AC.DIR))
    assert names == AC.FILES
    for n in names:
        assert os.path.getsize(os.path.join(AC.DIR, n)) <= AC.MAX_BYTES, n
        z = np.load(os.path.join(AC.DIR, n), allow_pickle=False)
        assert all(z[k].dtype.kind in "fiub" for k in z.files), n
