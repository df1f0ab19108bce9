"""Cross-talk FFN (node2edge_xtalk / edge2node_xtalk), the parts that need no GPU:

  * oracle pin     the fp64 restatement of tests/xtalk_cases.py against what the reference's own model code computed
                   (tests/golden/xtalk/*.npz), by the rule of tests/test_reference_exec_cpu.py: |a - r| <= 1e-12 max|r| per
                   tensor (absolute 1e-12 for an analytically zero tensor); regenerated where the reference tree is present
  * refusal tables egt_xtalk_supported over the geometry table; every refusal of the entry points by code and message, before
                   any launch (dummy pointers)
  * the models     fnn_lr2 shapes, Keras names, fraction 0 = today's model, the config keys
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import reference_cases as RC
import xtalk_cases as XC
from oracle import ref_exec as RX
from test_reference_exec_cpu import _bound, _check_values, needs_reference


# ----------------------------------------------------------------------------------------------- oracle pin -----
@pytest.mark.parametrize("name", list(XC.MODEL_CASES))
def test_restatement_matches_the_committed_reference_result(name):
    fix = XC.load(name)
    out, bits = XC.oracle_model(name)
    assert set(out) == set(fix["stat"]), set(out) ^ set(fix["stat"])
    for k, v in out.items():
        s, ss, mx = fix["stat"][k]
        _check_values(f"{name}: {k}", RC.picked(fix, k, v).numpy(), fix[f"out/{k}"], mx)
        whole = v.detach().double().reshape(-1)
        n = max(whole.numel(), 1)
        assert abs(float(whole.sum()) - s) <= n * _bound(mx), f"{name}: sum of {k}"
        assert abs(float((whole * whole).sum()) - ss) <= 2 * n * _bound(mx) * max(mx, 1.0), f"{name}: sum of squares of {k}"
    assert {k[5:] for k in fix["sha"] if k.startswith("bits/")} == set(bits)
    for k, v in bits.items():
        assert np.array_equal(RC.sha(v), fix["sha"][f"bits/{k}"]), f"{name}: {k} is not bit-equal"


def test_the_exchange_changes_the_numbers():
    """the fixtures are not those of the model without the keys: the restatement with both fractions 0 misses them"""
    name = "de16_both"
    fix = XC.load(name)
    inp, params, cfg = XC.model_inputs(name)
    with pytest.raises(RuntimeError):   # fnn_lr2 has the exchanged width: the plain FFN cannot even multiply
        XC.model_forward(inp, {k: t.double() for k, t in params.items()}, dict(cfg, node2edge_xtalk=0., edge2node_xtalk=0.))
    assert abs(float(fix["out/loss"][0])) > 0


def test_fixture_sizes():
    sizes = [os.path.getsize(XC.fixture_path(n)) for n in XC.MODEL_CASES]
    assert sorted(os.listdir(XC.XT_DIR)) == sorted(f"{n}.npz" for n in XC.MODEL_CASES)
    assert max(sizes) <= 128 * 1024, max(sizes)


def test_hidden_widths_of_the_cases():
    assert XC.widths(16, 64, .25, .25)[2:] == (100, 40)
    assert XC.widths(16, 64, .25, 0.)[2:] == (96, 48)
    assert XC.widths(16, 64, 0., .5)[2:] == (136, 16)


@needs_reference
@pytest.mark.parametrize("name", list(XC.MODEL_CASES))
def test_regenerated_fixture_equals_the_committed_one(name):
    with RX.reference() as R:
        case = XC.ref_model(R, name)
    new, old = RC.pack(case, XC.MODEL_CAP), XC.load(name)
    new_sha = dict(zip(new["sha_names"].tolist(), new["sha"]))
    assert set(new_sha) == set(old["sha"])
    for k, d in new_sha.items():
        assert np.array_equal(d, old["sha"][k]), f"{k} changed"
    for k in new["stat_names"].tolist():
        _check_values(f"{k} (regenerated)", new[f"out/{k}"], old[f"out/{k}"], old["stat"][k][2])
    out, _ = XC.oracle_model(name)
    for k, v in out.items():   # the restatement against the WHOLE tensors of the live reference run
        r = case["out"][k].detach().as_subclass(torch.Tensor).double()
        _check_values(f"{k} (whole tensor)", v.detach().double().numpy(), r.numpy(), float(r.abs().max()) if r.numel() else 0.0)


# ------------------------------------------------------------------------------------------- refusal tables -----
def _desc(**kw):
    from egt_amd import _lib as L
    d = dict(B=2, N=9, De=16, Dh=64, s_e=4, s_n=16, dtype=L.EGT_F32, activation=L.ACT_ELU, ln_eps=1e-3, flags=0, reserved=0)
    d.update(kw)
    return L.XtalkDesc(**d)


# the minimum the library covers: De 16 / 32 / 64, node widths 48 / 64, any N, s a multiple of 4 with 2 s <= H, either side 0
COVERED = [dict(De=De, Dh=Dh, N=N, s_e=s_e, s_n=s_n)
           for De in (16, 32, 64) for Dh in (48, 64) for N in (1, 9, 37, 300)
           for s_e in (0, 4, De // 2, De) for s_n in (0, 4, 12, 32, Dh)
           if (s_e or s_n) and 2 * De - 2 * s_e + s_n > 0]
REFUSED = [
    (dict(dtype=1), "DTYPE", "fp32 edge tensors"),
    (dict(flags=1), "FLAGS", "flags and reserved must be 0"),
    (dict(reserved=2), "FLAGS", "flags and reserved must be 0"),
    (dict(activation=0), "FLAGS", "EGT_ACT_RELU or EGT_ACT_ELU"),
    (dict(activation=1), "FLAGS", "EGT_ACT_RELU or EGT_ACT_ELU"),
    (dict(B=0), "SHAPE", "B >= 1 and N >= 1"),
    (dict(N=0), "SHAPE", "B >= 1 and N >= 1"),
    (dict(De=8), "SHAPE", "De in {16, 32, 64}"),
    (dict(De=48), "SHAPE", "De in {16, 32, 64}"),
    (dict(Dh=32), "SHAPE", "node widths 48 and 64"),
    (dict(s_e=6), "SHAPE", "s_e must be a multiple of 4"),
    (dict(s_e=20), "SHAPE", "s_e must be a multiple of 4 with 2 s_e <= 2 De"),
    (dict(s_e=-4), "SHAPE", "s_e must be a multiple of 4"),
    (dict(s_n=10), "SHAPE", "s_n must be a multiple of 4"),
    (dict(s_n=68), "SHAPE", "s_n must be a multiple of 4 with 2 s_n <= 2 Dh"),
    (dict(Dh=48, s_n=52), "SHAPE", "2 s_n <= 2 Dh"),
    (dict(s_e=0, s_n=0), "SHAPE", "no cross-talk"),
    (dict(s_e=16, s_n=0), "SHAPE", "fnn_lr2_edge would have no input"),
]


def test_supported_over_the_geometry_table(egt_lib):
    for kw in COVERED:
        d = _desc(**kw)
        assert egt_lib.egt_xtalk_supported(C.byref(d)) == 1, kw
        assert egt_lib.egt_xtalk_workspace_bytes(C.byref(d)) > 0, kw
    for kw, _, _ in REFUSED:
        d = _desc(**kw)
        assert egt_lib.egt_xtalk_supported(C.byref(d)) == 0, kw
        assert egt_lib.egt_xtalk_workspace_bytes(C.byref(d)) == 0, kw
    assert egt_lib.egt_xtalk_supported(None) == 0


@pytest.mark.parametrize("kw,code,text", REFUSED, ids=[f"{'-'.join(f'{k}{v}' for k, v in kw.items())}" for kw, _, _ in REFUSED])
def test_entry_points_refuse_by_code_and_message(kw, code, text, egt_lib):
    from egt_amd import _lib as L
    d, dummy = _desc(**kw), C.c_void_p(0x1000)
    pst = L.FfnParams(*([0x1000] * 6))
    want = getattr(L, "EGT_E_" + code)
    rc = egt_lib.egt_xtalk_fwd(C.byref(d), C.byref(pst), dummy, dummy, dummy, dummy, dummy, dummy, dummy, None)
    assert rc == want and text in egt_lib.egt_last_error_string().decode(), (rc, egt_lib.egt_last_error_string())
    rc = egt_lib.egt_xtalk_bwd(C.byref(d), C.byref(pst), dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy,
                               C.byref(pst), dummy, None)
    assert rc == want and text in egt_lib.egt_last_error_string().decode(), (rc, egt_lib.egt_last_error_string())


def test_entry_points_refuse_null_pointers(egt_lib):
    """every required pointer, NULL in turn: EGT_E_NULL before any launch"""
    from egt_amd import _lib as L
    d, x = _desc(), 0x1000
    full = L.FfnParams(*([x] * 6))
    fwd = [x] * 7            # e, mask, hr, hc, e_out, hn, workspace
    for i in range(7):
        a = [C.c_void_p(v) for v in fwd]
        a[i] = None
        assert egt_lib.egt_xtalk_fwd(C.byref(d), C.byref(full), *a, None) == L.EGT_E_NULL, i
    bwd = [x] * 9            # e, mask, hr, hc, d_e_out, d_hn, d_e, d_hr, d_hc
    for i in range(9):
        a = [C.c_void_p(v) for v in bwd]
        a[i] = None
        assert egt_lib.egt_xtalk_bwd(C.byref(d), C.byref(full), *a, C.byref(full), C.c_void_p(x), None) == L.EGT_E_NULL, i
    for f in L.FFN_PARAM_FIELDS:
        hole = L.FfnParams(*([x] * 6))
        setattr(hole, f, None)
        a = [C.c_void_p(v) for v in fwd]
        assert egt_lib.egt_xtalk_fwd(C.byref(d), C.byref(hole), *a, None) == L.EGT_E_NULL, f
        b = [C.c_void_p(v) for v in bwd]
        assert egt_lib.egt_xtalk_bwd(C.byref(d), C.byref(full), *b, C.byref(hole), C.c_void_p(x), None) == L.EGT_E_NULL, f
    assert egt_lib.egt_xtalk_fwd(None, C.byref(full), *[C.c_void_p(v) for v in fwd], None) == L.EGT_E_NULL


def test_one_sided_calls_take_null_for_the_absent_side(egt_lib):
    """s_n = 0: hr / hc may be NULL; the first complaint is then about something else (here: the workspace)"""
    from egt_amd import _lib as L
    d, x = _desc(s_n=0), C.c_void_p(0x1000)
    full = L.FfnParams(*([0x1000] * 6))
    rc = egt_lib.egt_xtalk_fwd(C.byref(d), C.byref(full), x, x, None, None, None, x, x, None)
    assert rc == L.EGT_E_NULL and "e_out" in egt_lib.egt_last_error_string().decode()


def test_abi_version_is_unchanged(egt_lib):
    assert egt_lib.egt_abi_version() == 4


# ---------------------------------------------------------------------------------------------- the models -----
def _small(cls, **kw):
    base = dict(model_width=64, edge_width=16, model_height=2, upto_hop=4)
    base.update(kw)
    return cls(**base)


def _model_classes():
    from egt_amd.model import PatternDCTransformer, ZincDCTransformer
    return [ZincDCTransformer, PatternDCTransformer]


@pytest.mark.parametrize("n2e,e2n,edge,node", [(.25, .25, 40, 100), (.25, 0., 48, 96), (0., .5, 16, 136)])
def test_lr2_kernels_have_the_exchanged_widths(n2e, e2n, edge, node, egt_lib):
    for cls in _model_classes():
        m = _small(cls, node2edge_xtalk=n2e, edge2node_xtalk=e2n)
        named = m.layers.keras_named_parameters()
        for tag in ("00", "01"):
            assert tuple(named[f"fnn_lr2_edge_{tag}/kernel"].shape) == (edge, 16)
            assert tuple(named[f"fnn_lr2_node_{tag}/kernel"].shape) == (node, 64)
            assert tuple(named[f"fnn_lr1_edge_{tag}/kernel"].shape) == (16, 32)
            assert tuple(named[f"fnn_lr1_node_{tag}/kernel"].shape) == (64, 128)


def test_keras_names_do_not_change_and_dead_parameters_follow_the_reference(egt_lib):
    from egt_amd.model import ZincDCTransformer
    plain = _small(ZincDCTransformer)
    both = _small(ZincDCTransformer, node2edge_xtalk=.25, edge2node_xtalk=.25)
    n2e = _small(ZincDCTransformer, node2edge_xtalk=.25)
    assert set(plain.layers.keras_named_parameters()) == set(both.layers.keras_named_parameters())
    # readout_edges=False: without edge -> node cross-talk the last layer's edge side is dead, as in the plain model; with it
    # the last fnn_lr1_edge feeds the nodes (the fixtures: non-zero gradients) and only fnn_lr2_edge is dead
    assert set(n2e.keras_named_parameters()) == set(plain.keras_named_parameters())
    extra = set(both.keras_named_parameters()) - set(plain.keras_named_parameters())
    assert extra == {"dense_edge_r_01/kernel", "dense_edge_r_01/bias", "norm_fnn_edge_01/gamma", "norm_fnn_edge_01/beta",
                     "fnn_lr1_edge_01/kernel", "fnn_lr1_edge_01/bias"}
    fix = XC.load("de16_both")
    live = {RC.keras_name(k[2:]) for k in fix["stat"] if k.startswith("d/") and fix["stat"][k][2] > 1e-9}
    mine = {k for k in both.keras_named_parameters() if k.split("/")[0].endswith(("_00", "_01"))}
    assert {k for k in live if k.split("/")[0].endswith(("_00", "_01"))} <= mine
    assert not ({"fnn_lr2_edge_01/kernel", "fnn_lr2_edge_01/bias"} & live)


def test_fraction_zero_is_todays_model(egt_lib):
    from egt_amd import fused as FZ
    from egt_amd.ffn import FFN
    from egt_amd.model import ZincDCTransformer
    torch.manual_seed(3)
    a = _small(ZincDCTransformer)
    torch.manual_seed(3)
    b = _small(ZincDCTransformer, node2edge_xtalk=0., edge2node_xtalk=0.)
    assert b.layers.xtalk is None and all(isinstance(f, FFN) for f in list(b.layers.ffn_node) + list(b.layers.ffn_edge))
    pa, pb = a.keras_named_parameters(), b.keras_named_parameters()
    assert list(pa) == list(pb) and all(torch.equal(pa[k], pb[k]) for k in pa)
    for blk_a, blk_b in zip(a.layers.blocks, b.layers.blocks):
        for on_gpu in (False, True):
            assert FZ.route_core(blk_a, 2, 9, torch.float32, torch.float32, on_gpu) == \
                FZ.route_core(blk_b, 2, 9, torch.float32, torch.float32, on_gpu)


def test_bias_edge_channels_are_the_unchanged_model(egt_lib):
    from egt_amd.model import ZincDCTransformer
    torch.manual_seed(5)
    a = _small(ZincDCTransformer, edge_channel_type="bias", edge_width=8)
    torch.manual_seed(5)
    b = _small(ZincDCTransformer, edge_channel_type="bias", edge_width=8, node2edge_xtalk=.25, edge2node_xtalk=.25)
    assert b.layers.xtalk is None and b.layers.ffn_edge is None
    pa, pb = a.keras_named_parameters(), b.keras_named_parameters()
    assert list(pa) == list(pb) and all(torch.equal(pa[k], pb[k]) for k in pa)


@pytest.mark.parametrize("kw", [dict(edge_dtype="bf16"), dict(num_virtual_nodes=1)])
def test_what_is_not_built_says_so(kw, egt_lib):
    from egt_amd.model import ZincDCTransformer
    with pytest.raises(NotImplementedError, match="covers the shipped configs; not built"):
        _small(ZincDCTransformer, node2edge_xtalk=.25, **kw)


def test_fraction_validation(egt_lib):
    from egt_amd.model import ZincDCTransformer
    for bad in (-.1, 1.5, "a", True):
        with pytest.raises(ValueError, match="fraction"):
            _small(ZincDCTransformer, edge2node_xtalk=bad)
    with pytest.raises(ValueError, match="ffn_multiplier = 2"):
        _small(ZincDCTransformer, node2edge_xtalk=.25, ffn_matmul="bf16x3")


def test_composed_op_is_the_restatement_in_fp64():
    """xtalk_ffn_composed (the fallback of the models) against the test helpers' restatement, both in fp64 on the CPU"""
    from egt_amd.xtalk import xtalk_ffn_composed
    for name in ("n9_de16", "n33_de16_empty", "n19_de32_n2e", "n37_de64_e2n"):
        c, inp, pn, pe = XC.op_inputs(name)
        ref = XC.op_reference(name)
        h2, e2 = xtalk_ffn_composed(inp["h"].double(), inp["e"].double(), inp["mask"], [pn[k].double() for k in XC.FFN_NAMES],
                                    [pe[k].double() for k in XC.FFN_NAMES], c["n2e"], c["e2n"], c["act"])
        assert float((h2 - ref["h_out"]).abs().max()) <= 1e-12 * float(ref["h_out"].abs().max())
        assert float((e2 - ref["e_out"]).abs().max()) <= 1e-12 * float(ref["e_out"].abs().max())


def test_no_cpu_path_to_the_fused_op():
    from egt_amd.xtalk import xtalk_ffn
    c, inp, pn, pe = XC.op_inputs("n9_de16")
    with pytest.raises(RuntimeError, match="no CPU path"):
        xtalk_ffn(inp["h"], inp["e"], inp["mask"], [pn[k] for k in XC.FFN_NAMES], [pe[k] for k in XC.FFN_NAMES], .25, .25)


# --------------------------------------------------------------------------------------------- config keys -----
def test_config_keys():
    from egt_amd import training as T
    base = T.model_config(T.make_config({}, "zinc.svd"))
    assert "node2edge_xtalk" not in base and "edge2node_xtalk" not in base
    assert T.model_config(T.make_config(dict(node2edge_xtalk=0., edge2node_xtalk=0.), "zinc.svd")) == base
    mc = T.model_config(T.make_config(dict(node2edge_xtalk=.25), "zinc.svd"))
    assert mc == dict(base, node2edge_xtalk=.25)
    mc = T.model_config(T.make_config(dict(node2edge_xtalk=.25, edge2node_xtalk=.5), "pattern.svd"))
    assert mc["node2edge_xtalk"] == .25 and mc["edge2node_xtalk"] == .5
    for bad in (-1, 2, "x", True, None):
        with pytest.raises(ValueError, match="fraction"):
            T.make_config(dict(edge2node_xtalk=bad), "zinc.svd")
