"""Degree scalers on the fused block, pinned without a GPU (library built): the route table of egt_amd.fused.route_core for blocks
with scale_degree, the library's answers and flag checks for descriptors with EGT_BF_SCALE_DEGREE / EGT_BF_SCALER_LINEAR, and the
fairness of the "small degree" recipe of tests/test_scale_degree_gpu.py, checked with the fp64 oracle."""
import ctypes as C

import pytest
import torch

from test_fused_host_cpu import _call, _desc, ENTRIES, RES, BIAS, COMPOSED, NARROW, EDGE_DTYPE, _case, make_block

SD = dict(scale_degree=True)
ROUTE_CASES = [
    _case(f"sd_{t}_De{De}", RES, model_width=Dh, edge_width=De, scaler_type=t, **SD)
    for t in ("log", "linear") for Dh, De in ((64, 64), (48, 48), (64, 8))
] + [
    _case("sd_constrained_mask", RES, attn_mask=True, edge_channel_type="constrained", **SD),
    _case("sd_train_in_kernel_mask", RES, train=True, random_mask_prob=0.1, **SD),
    _case("sd_host_rand_mask", RES, rand_mask=True, train=True, random_mask_prob=0.1, **SD),
    _case("sd_bias_in_stack_De8", BIAS, in_stack=True, edge_channel_type="bias", **SD, **NARROW),   # never "static"
    _case("sd_bias_alone_De8", BIAS, edge_channel_type="bias", **SD, **NARROW),
    _case("sd_bf16", COMPOSED, edge="bf16", **SD),
    _case("sd_bf16_De8", COMPOSED, edge="bf16", **SD, **NARROW),
    _case("sd_virtual_nodes", COMPOSED, num_virtual_nodes=2, **SD),
    _case("sd_width512_pair_geometry", COMPOSED, N=16, model_width=512, edge_width=32, **SD),
    _case("sd_bf16_fused_true", RuntimeError, edge="bf16", fused=True, **SD),
]


@pytest.fixture
def sd_switch():
    """EGT_NO_SCALE_DEGREE is read once per process: set the remembered answer for a case, restore it afterwards"""
    from egt_amd import fused as FZ
    old = FZ._NO_SCALE_DEGREE

    def set_(off):
        FZ._NO_SCALE_DEGREE = bool(off)
    yield set_
    FZ._NO_SCALE_DEGREE = old


def _route(case):
    from egt_amd import fused as FZ
    blk = make_block(case)
    args = (blk, 2, case["N"], torch.float32, EDGE_DTYPE[case["edge"]], True)
    return FZ.route_core(*args, attn_mask=case["attn_mask"], rand_mask=case["rand_mask"], training=case["train"])


@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: c["name"])
def test_route_table(egt_lib, sd_switch, case):
    sd_switch(False)
    if case["want"] is RuntimeError:
        with pytest.raises(RuntimeError, match="not covered"):
            _route(case)
        return
    assert _route(case) == case["want"]


@pytest.mark.parametrize("case", [c for c in ROUTE_CASES if c["want"] in (RES, BIAS)], ids=lambda c: c["name"])
def test_switch_sends_every_case_to_the_composed_route(egt_lib, sd_switch, case):
    sd_switch(True)
    assert _route(case) == COMPOSED


def test_stack_call_is_not_taken(egt_lib):
    """egt_stack_* refuses the flag, so an EGTStack of such blocks runs block by block (fused.stack_supported)"""
    from egt_amd import fused as FZ
    from egt_amd.layers import EGTStack
    st = EGTStack(model_height=2, model_width=64, edge_width=64, num_heads=8, scale_degree=True)
    h = torch.zeros(2, 19, 64); e = torch.zeros(2, 19, 19, 64)
    assert FZ.stack_supported(st, h, e, None) is False


def test_unsupported_messages(egt_lib, sd_switch):
    from egt_amd import fused as FZ
    from egt_amd.layers import EGTBlock
    sd_switch(False)
    assert FZ._unsupported(EGTBlock(model_width=64, edge_width=64, scale_degree=True), True) is None
    assert "scale_degree with virtual nodes" in FZ._unsupported(EGTBlock(model_width=64, edge_width=64, scale_degree=True, num_virtual_nodes=2), True)
    # the messages existing tests match substrings of
    assert FZ._unsupported(EGTBlock(model_width=64, edge_width=64, num_virtual_nodes=1), True) == "scale_degree / attn_dropout / virtual nodes"
    assert FZ._unsupported(EGTBlock(model_width=64, edge_width=64, scale_degree=True, attn_dropout=0.1), True) == "scale_degree / attn_dropout / virtual nodes"
    why = FZ.bf16_refusal(EGTBlock(model_width=64, edge_width=64, scale_degree=True))
    assert why is not None and "scale_degree" in why and "bf16" in why
    sd_switch(True)
    assert "EGT_NO_SCALE_DEGREE" in FZ._unsupported(EGTBlock(model_width=64, edge_width=64, scale_degree=True), True)


# ----------------------------------------------------------------------------------------- the library's answers -----
def _sd(L, De=64, flags=0, dtype=None, N=19, d=8, B=2):
    desc = _desc(L, De=De, flags=L.BF_SCALE_DEGREE | flags)
    desc.N, desc.d, desc.B = N, d, B
    if dtype is not None:
        desc.dtype = dtype
    return desc


def test_library_answers(egt_lib):
    from egt_amd import _lib as L
    lib = egt_lib
    for De in (8, 16, 32, 48, 64):
        for lin in (0, L.BF_SCALER_LINEAR):
            for extra in (0, L.BF_ATTN_MASK, L.BF_TRAINING, L.BF_NO_EDGE_LN):
                d = _sd(L, De=De, flags=lin | extra)
                assert lib.egt_block_supported(C.byref(d)) == 1, (De, lin, extra)
                assert lib.egt_pair_supported(C.byref(d)) == 0
    assert lib.egt_block_supported(C.byref(_sd(L, dtype=L.EGT_BF16))) == 0
    assert lib.egt_block_supported(C.byref(_sd(L, De=8, flags=L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN))) == 0
    # the pair operator's own geometry (d = 64, De = 32): covered without the flag, not with it
    plain = _desc(L, De=32); plain.d, plain.N = 64, 16
    assert lib.egt_pair_supported(C.byref(plain)) == 1
    flagged = _sd(L, De=32, d=64, N=16)
    assert lib.egt_pair_supported(C.byref(flagged)) == 0 and lib.egt_block_supported(C.byref(flagged)) == 0


@pytest.mark.parametrize("N,B", [(19, 2), (69, 2), (150, 2), (120, 16)])
def test_de8_runs_on_the_mfma_tile_kernels(egt_lib, N, B):
    """with the flag De = 8 takes k_block_fwd_r4 / k_block_bwd_v4r (egt_narrow.hip has no degree), as under EGT_NO_NARROW=1"""
    from egt_amd import _lib as L
    d = _sd(L, De=8, N=N, B=B)
    form = egt_lib.egt_block_launch_form(C.byref(d)).decode()
    assert form.startswith("fwd=k_block_fwd_r4/") and " bwd=k_block_bwd_v4r/4w/" in form, form
    assert egt_lib.egt_block_bwd_kernel(C.byref(d)).decode() == "k_block_bwd_v4r"
    plain = _desc(L, De=8); plain.N, plain.B = N, B
    assert "k_narrow" in egt_lib.egt_block_launch_form(C.byref(plain)).decode()      # (the unflagged plan is untouched)


@pytest.mark.parametrize("De,N,fwd,bwd", [(64, 64, "k_block_fwd/", "k_block_bwd_v5"), (48, 37, "k_block_fwd/", "k_block_bwd_v5"),
                                          (16, 80, "k_block_fwd_r4/", "k_block_bwd_v4r"), (32, 21, "k_block_fwd/", "k_block_bwd_v5")])
def test_launch_forms_and_sizes_equal_the_unflagged_descriptor(egt_lib, De, N, fwd, bwd):
    from egt_amd import _lib as L
    for mask in (0, L.BF_ATTN_MASK):
        a = _desc(L, De=De, flags=mask); a.N = N
        b = _sd(L, De=De, N=N, flags=mask | L.BF_SCALER_LINEAR)
        assert egt_lib.egt_block_saved_bytes(C.byref(a)) == egt_lib.egt_block_saved_bytes(C.byref(b)) > 0
        assert egt_lib.egt_block_workspace_bytes(C.byref(a)) == egt_lib.egt_block_workspace_bytes(C.byref(b)) > 0
        fa, fb = egt_lib.egt_block_launch_form(C.byref(a)).decode(), egt_lib.egt_block_launch_form(C.byref(b)).decode()
        assert fa == fb and (mask or (f"fwd={fwd}" in fb and f"bwd={bwd}/" in fb)), (fa, fb)
        if mask:
            assert egt_lib.egt_block_bwd_kernel(C.byref(b)).decode() == "k_block_bwd_v4"
    # De = 8: same buffers as the unflagged descriptor although other kernels run
    a = _desc(L, De=8); b = _sd(L, De=8)
    assert egt_lib.egt_block_saved_bytes(C.byref(a)) == egt_lib.egt_block_saved_bytes(C.byref(b)) > 0
    assert egt_lib.egt_block_workspace_bytes(C.byref(a)) == egt_lib.egt_block_workspace_bytes(C.byref(b)) > 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_flag_rules(egt_lib, entry):
    from egt_amd import _lib as L
    stack = entry.startswith("egt_stack")

    def expect(code, text, desc):
        rc, msg = _call(egt_lib, L, entry, desc)
        assert rc == code and text in msg, (entry, rc, msg)

    if stack:      # refused like EGT_BF_STATIC_EDGE, flags before pointers and sizes
        expect(L.EGT_E_FLAGS, "egt_stack_* does not take EGT_BF_SCALE_DEGREE", _sd(L))
        expect(L.EGT_E_FLAGS, "egt_stack_* does not take EGT_BF_SCALE_DEGREE", _sd(L, flags=L.BF_SCALER_LINEAR))
        d = _sd(L)
        assert egt_lib.egt_stack_saved_bytes(C.byref(d), 2) == 0 and egt_lib.egt_stack_workspace_bytes(C.byref(d), 2) == 0
        return
    ungated = _sd(L); ungated.flags &= ~L.BF_GATE
    expect(L.EGT_E_FLAGS, "EGT_BF_SCALE_DEGREE needs EGT_BF_GATE", ungated)
    expect(L.EGT_E_FLAGS, "EGT_BF_SCALER_LINEAR is only valid together with EGT_BF_SCALE_DEGREE", _desc(L, flags=L.BF_SCALER_LINEAR))
    expect(L.EGT_E_FLAGS, "EGT_BF_SCALE_DEGREE does not take EGT_BF_STATIC_EDGE", _sd(L, De=8, flags=L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN))
    rc, msg = _call(egt_lib, L, entry, _sd(L, dtype=L.EGT_BF16))
    assert rc != L.EGT_OK and "EGT_BF_SCALE_DEGREE with bf16 edge tensors is not covered" in msg, (rc, msg)


# --------------------------------------------------------------------------------- fairness of the GPU recipes -----
@pytest.mark.parametrize("shape", ["n19_de64", "n37_d6_de48", "n69_de8"])
def test_small_degree_recipe(shape):
    """tests/test_scale_degree_gpu.py::test_small_degree: with attention_gates.bias[0] = -12 head 0's degree lies in (1e-6, 1e-2)
    on every real row -- where log(1 + deg) must be a log1p -- and the other heads' degrees are above 1; every gradient of the
    oracle is finite there"""
    import scale_degree_cases as G
    from oracle import egt_oracle as O
    B, N, d, De, nodes, _, _ = G.SHAPES[shape]
    inp, params, attrs, c = G.make_case(B, N, d, De, nodes, shape, gate_bias0=-12.0)
    p = {k: v.double() for k, v in params.items()}
    ehat = O.layer_norm(inp["e"].double(), p["norm_edge.gamma"], p["norm_edge.beta"])
    gl = O.dense(ehat, p["attention_gates.kernel"], p["attention_gates.bias"])               # [B, N, N, H]
    mask = inp["mask"]
    gate = torch.sigmoid(gl) * mask[:, None, :, None]
    deg = gate.sum(2)                                                                         # [B, N, H]
    real = deg[mask]                                                                          # rows of real nodes
    assert 1e-6 < float(real[:, 0].min()) and float(real[:, 0].max()) < 1e-2, (float(real[:, 0].min()), float(real[:, 0].max()))
    assert float(real[:, 1:].min()) > 1.0, float(real[:, 1:].min())
    for scaler in ("log", "linear"):
        ref = G.oracle(inp, params, attrs, scaler)
        for k in ("h_out", "e_out", "dh", "de"):
            assert torch.isfinite(ref[k]).all(), k
        assert all(torch.isfinite(g).all() for g in ref["dparams"].values())


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


@pytest.mark.parametrize("scaler", ["log", "linear"])
def test_oracle_equals_the_reference_block_fixture(scaler):
    import scale_degree_cases as SC
    fix = SC.load(f"block_{scaler}.npz")
    inp, params, _ = SC.block_inputs(scaler)
    for k, v in list(inp.items()) + list(params.items()):      # the stored inputs and weights ARE the seeded recipe's
        if v is not None:
            grp = "weights" if k in params else "inputs"
            assert (torch.from_numpy(fix[f"{grp}/{k}"]) == v).all(), k
    _oracle_equals(SC.load_out(f"block_{scaler}.npz"), SC.oracle_block(scaler), f"block_{scaler}")


def test_oracle_equals_the_reference_model_fixture():
    import scale_degree_cases as SC
    fix = SC.load("model_zinc.npz")
    inp, params, _ = SC.model_inputs()
    for k, v in inp.items():
        assert (torch.from_numpy(fix[f"inputs/{k}"]) == v).all(), k
    for k, v in params.items():
        assert (torch.from_numpy(fix[f"weights/{k}"]) == v).all(), k
    ref = SC.load_out("model_zinc.npz", "model_zinc_grads.npz")
    assert set(ref) == {"y", "loss"} | {f"d/{k}" for k in params}      # prediction, loss and EVERY weight gradient
    _oracle_equals(ref, SC.oracle_model(), "model_zinc")


def test_fixture_files_are_small_and_hold_data_only():
    import os
    import numpy as np
    import scale_degree_cases as SC
    names = sorted(os.listdir(SC.DIR))
    assert names == ["block_linear.npz", "block_log.npz", "model_zinc.npz", "model_zinc_grads.npz"]
    for n in names:
        assert os.path.getsize(os.path.join(SC.DIR, n)) <= SC.MAX_BYTES, n
        z = np.load(os.path.join(SC.DIR, n), allow_pickle=False)
        assert all(z[k].dtype.kind in "fiub" for k in z.files), n


def test_new_flags_header_and_ctypes_agree():
    """the two new bits of egt_block_desc.flags (written as shifts in the header), their Python mirror, no overlap with the
    existing flags, and the ABI version, which stays 4 (no struct changes layout)"""
    import os
    import re
    from egt_amd import _lib as L
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egt_amd.h")).read()
    shifts = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"#define EGT_BF_([A-Z_]+) \(1u << (\d+)\)", src)}
    assert shifts == dict(SCALE_DEGREE=L.BF_SCALE_DEGREE, SCALER_LINEAR=L.BF_SCALER_LINEAR) == dict(SCALE_DEGREE=0x80, SCALER_LINEAR=0x100)
    old = [int(m.group(1), 16) for m in re.finditer(r"#define EGT_BF_[A-Z_]+ (0x[0-9a-fA-F]+)u", src)]
    assert not (sum(old) & (0x80 | 0x100)) and len(set(old)) == len(old)
    assert re.search(r"#define EGT_ABI_VERSION (\d+)", src).group(1) == str(L.ABI_VERSION) == "4"
