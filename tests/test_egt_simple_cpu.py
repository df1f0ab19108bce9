"""EGT-Simple ('bias' edge channels, the reference's configs/ablation/egt_simple family) without a GPU: the models build with
exactly the reference's Keras variables, the five width-64 configs load through the scheme driver, the C-ABI flag of the
static-edge mode is mirrored and answered for by the library, and the test-side oracle composition reproduces its golden."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import egt_simple_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "egt_simple", "*.json")))


def expected_names(kind, Ly, gated=True, mlp=2):
    """the Keras variables the reference builds for edge_channel_type='bias' (graph_xformer_model_base.py:173-190, :309-324)"""
    per_layer = (["attention_gates_{t}/kernel", "attention_gates_{t}/bias"] if gated else []) + [
        "dense_edge_b_{t}/kernel", "dense_edge_b_{t}/bias", "norm_mha_{t}/gamma", "norm_mha_{t}/beta",
        "dense_qkv_{t}/kernel", "dense_qkv_{t}/bias", "dense_mha_{t}/kernel", "dense_mha_{t}/bias",
        "norm_fnn_node_{t}/gamma", "norm_fnn_node_{t}/beta", "fnn_lr1_node_{t}/kernel", "fnn_lr1_node_{t}/bias",
        "fnn_lr2_node_{t}/kernel", "fnn_lr2_node_{t}/bias"]
    names = {n.format(t=f"{i:0>2d}") for i in range(Ly) for n in per_layer}
    names |= {"adj_emb/kernel", "adj_emb/bias", "node_norm_final/gamma", "node_norm_final/beta", "target/kernel", "target/bias"}
    names |= {f"mlp_out_{i}/{a}" for i in range(mlp) for a in ("kernel", "bias")}
    if kind == "zinc":
        names |= {"node_emb/embeddings", "fm_emb/embeddings"}
    elif kind == "pattern":
        names |= {"node_emb/embeddings"}
    else:
        names |= {"node_emb/kernel", "node_emb/bias", "edge_emb/kernel", "edge_emb/bias"}
    return names


def expected_count(kind, Dh, De, Ly, K, H=8, gated=True, targets=1, mult=2.0, node_feats=28, edge_feats=4):
    """parameter count from the config by the Keras layer list (Dense = in * out + out, LayerNormalization = 2 * width)"""
    dense = lambda i, o: i * o + o
    hid = round(Dh * mult)
    layer = (dense(De, H) if gated else 0) + dense(De, H) + 2 * Dh + dense(Dh, 3 * Dh) + dense(Dh, Dh) \
        + 2 * Dh + dense(Dh, hid) + dense(hid, Dh)
    n = Ly * layer + dense(K, De) + 2 * Dh + dense(Dh, Dh // 2) + dense(Dh // 2, Dh // 4) + dense(Dh // 4, targets)
    if kind == "zinc":
        n += (node_feats + 1) * Dh + (edge_feats + 1) * De
    elif kind == "pattern":
        n += (3 + 1) * Dh
    else:
        n += dense(5, Dh) + dense(1, De)
    return n


@pytest.mark.parametrize("kind,gated", [("zinc", True), ("pattern", True), ("cifar10", True), ("pattern", False)])
def test_models_build_with_bias_edge_channels(kind, gated):
    from egt_amd import ZincDCTransformer, PatternDCTransformer, Cifar10DCTransformer
    cls = dict(zinc=ZincDCTransformer, pattern=PatternDCTransformer, cifar10=Cifar10DCTransformer)[kind]
    Ly, Dh, De, K = 3, 64, 8, 16
    m = cls(model_width=Dh, edge_width=De, model_height=Ly, upto_hop=K, edge_channel_type="bias", gate_attention=gated)
    named = m.keras_named_parameters()
    assert set(named) == expected_names(kind, Ly, gated)
    for frag in ("norm_edge", "dense_edge_r", "_edge_0", "edge_norm_final"):
        assert not [k for k in named if frag in k and not k.startswith("dense_edge_b")], frag
    targets = dict(zinc=1, pattern=2, cifar10=10)[kind]
    assert sum(p.numel() for p in named.values()) == expected_count(kind, Dh, De, Ly, K, gated=gated, targets=targets)
    assert m._dead_edge_params() == []
    assert {id(p) for p in m.parameters()} == {id(p) for p in named.values()}       # the module owns nothing else
    assert m.layers.ffn_edge is None and all(b._static_edge for b in m.layers.blocks)
    assert all(not hasattr(b, "norm_edge") and not hasattr(b, "dense_edge_r") for b in m.layers.blocks)


def test_bias_models_at_other_widths_and_refusals():
    from egt_amd import ZincDCTransformer
    m = ZincDCTransformer(model_width=64, edge_width=16, model_height=2, edge_channel_type="bias")   # per-block route
    assert "dense_edge_b_01/kernel" in m.keras_named_parameters()
    with pytest.raises(NotImplementedError, match="must be residual or constrained"):   # the ZINC egt_simple configs: d = 10
        ZincDCTransformer(model_width=80, edge_width=8, model_height=2, edge_channel_type="bias")
    with pytest.raises(NotImplementedError):
        ZincDCTransformer(model_width=64, edge_width=8, model_height=2, edge_channel_type="none")


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(p)[:-5] for p in CONFIGS])
def test_reference_egt_simple_configs_load(path):
    from egt_amd import training as T
    cfg = json.load(open(path))
    assert cfg["edge_channel_type"] == "bias" and cfg["edge_width"] == 8 and cfg["model_width"] == 64
    c = T.make_config(cfg)
    mc = T.model_config(c)
    assert mc["edge_channel_type"] == "bias"
    model = T.import_scheme(cfg["scheme"])(cfg).get_model()
    kind = "pattern" if cfg["scheme"].startswith("pattern") else "cifar10"
    names = set(model.keras_named_parameters())
    extra = {"svd_emb/kernel", "svd_emb/bias"} if (cfg.get("use_svd") and mc.get("transform_svd")) else set()
    assert names - extra == expected_names(kind, cfg["model_height"])
    assert model.layers.ffn_edge is None


def test_five_fixture_configs_are_present():
    assert [os.path.basename(p) for p in CONFIGS] == [
        "cifar10_100k_egt_simple.json", "cifar10_100k_egt_simple_spe.json", "pattern_500k_egt_simple.json",
        "pattern_500k_egt_simple_epe.json", "pattern_500k_egt_simple_spe.json"]


def test_static_edge_flag_header_and_ctypes_agree():
    from egt_amd import _lib as L
    src = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    flags = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define EGT_BF_([A-Z_]+) (0x[0-9a-fA-F]+)u", src)}
    assert flags["STATIC_EDGE"] == 0x40 == L.BF_STATIC_EDGE
    mirror = dict(GATE=L.BF_GATE, ATTN_MASK=L.BF_ATTN_MASK, TRAINING=L.BF_TRAINING, CLIP=L.BF_CLIP, NO_EDGE_LN=L.BF_NO_EDGE_LN,
                  SEED_DEVICE=L.BF_SEED_DEVICE, STATIC_EDGE=L.BF_STATIC_EDGE)
    assert flags == mirror
    assert re.search(r"#define EGT_ABI_VERSION (\d+)", src).group(1) == str(L.ABI_VERSION) == "4"


def _desc(L, flags, **kw):
    d = dict(B=4, N=37, H=8, d=8, De=8, dtype=L.EGT_F32, flags=flags, clip_lo=-5, clip_hi=5, random_mask_prob=0.0, ln_eps=1e-3,
             reserved=0, seed=0, seed_device=None)
    d.update(kw)
    return L.BlockDesc(**d)


def test_static_edge_descriptor_answers(egt_lib):
    """egt_block_supported with EGT_BF_STATIC_EDGE: 1 exactly where the De = 8 pair kernels run; the stack entry points
    refuse the flag with an error code (descriptor path only: no launch)."""
    from egt_amd import _lib as L
    SE = L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN | L.BF_GATE | L.BF_CLIP
    sup = lambda d: egt_lib.egt_block_supported(C.byref(d))
    for dt in (L.EGT_F32, L.EGT_BF16):
        for d in (6, 8):
            assert sup(_desc(L, SE, d=d, dtype=dt)) == 1
    assert sup(_desc(L, SE & ~L.BF_GATE & ~L.BF_CLIP)) == 1
    for De in (16, 32, 48, 64):
        assert sup(_desc(L, SE, De=De)) == 0
        assert sup(_desc(L, SE & ~L.BF_STATIC_EDGE, De=De)) == 1                     # without the flag nothing changes
    assert sup(_desc(L, SE | L.BF_ATTN_MASK)) == 0
    assert sup(_desc(L, SE & ~L.BF_NO_EDGE_LN)) == 0                                 # only valid with EGT_BF_NO_EDGE_LN
    assert sup(_desc(L, SE, d=16)) == 0 and sup(_desc(L, SE, H=4)) == 0
    d = _desc(L, SE)
    assert egt_lib.egt_block_bwd_kernel(C.byref(d)) == b"k_narrow_bwd"
    prm = L.BlockParams()
    assert egt_lib.egt_stack_saved_bytes(C.byref(d), 2) == 0 and egt_lib.egt_stack_workspace_bytes(C.byref(d), 2) == 0
    assert egt_lib.egt_stack_fwd(C.byref(d), 2, C.byref(prm), *([None] * 9)) == L.EGT_E_FLAGS
    assert b"EGT_BF_STATIC_EDGE" in egt_lib.egt_last_error_string()
    assert egt_lib.egt_stack_bwd(C.byref(d), 2, C.byref(prm), *([None] * 9), C.byref(prm), None, None) == L.EGT_E_FLAGS
    # egt_block_fwd: the flag combination is checked before anything is launched
    bad = _desc(L, SE & ~L.BF_NO_EDGE_LN)
    assert egt_lib.egt_block_fwd(C.byref(bad), C.byref(prm), *([None] * 10)) == L.EGT_E_FLAGS
    # same buffer sizes with and without the flag (one plan per geometry)
    plain = _desc(L, SE & ~L.BF_STATIC_EDGE)
    assert egt_lib.egt_block_saved_bytes(C.byref(d)) == egt_lib.egt_block_saved_bytes(C.byref(plain)) > 0
    assert egt_lib.egt_block_workspace_bytes(C.byref(d)) == egt_lib.egt_block_workspace_bytes(C.byref(plain)) > 0


def test_oracle_composition_reproduces_its_golden():
    out = R.small_case_outputs()
    gold = np.load(R.GOLDEN)
    assert set(gold.files) == set(out)
    for k in gold.files:
        np.testing.assert_allclose(out[k], gold[k], rtol=1e-9, atol=1e-12, err_msg=k)
    assert not [k for k in gold.files if "norm_edge" in k or "dense_edge_r" in k or "ffn_edge" in k or "edge_norm_final" in k]
    assert float(np.abs(gold["d/adj_emb.kernel"]).max()) > 0 and float(np.abs(gold["d/fm_emb.embeddings"]).max()) > 0


def test_oracle_composition_is_the_bias_loop():
    """the composition against a hand-written second form: dropping every layer's edge projections' input changes the
    prediction (e reaches h through every layer), and e itself is what the embedding made (never updated)"""
    cfg, inp, params = R.small_case()
    p = {k: v.double() for k, v in params.items()}
    y, mask = R.forward("zinc", inp, p, cfg)
    p2 = dict(p); p2["layer1.dense_edge_b.kernel"] = torch.zeros_like(p["layer1.dense_edge_b.kernel"])
    y2, _ = R.forward("zinc", inp, p2, cfg)
    assert not torch.allclose(y, y2)
    assert mask.sum(1).tolist() == [11, 6, 9]
