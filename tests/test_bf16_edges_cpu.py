"""bf16 edge tensors beyond the fused block (include/egt_amd.h EGT_BF16): what the channel FFN and the edge embedding
report for EGT_BF16 descriptors, their argument checks, and the training driver's edge_dtype key.  No GPU needed."""
import ctypes as C
import json
import os

import pytest

from egt_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {8: ("f32",), 16: ("f32", "bf16x3", "bf16"), 32: ("f32", "bf16x3", "bf16"), 48: ("f32", "bf16x3", "bf16"),
         64: ("f32", "bf16x3", "bf16")}


def _ffn(rows, width, dtype, matmul="f32", act="elu"):
    from egt_amd.ffn import _MM, _ACT
    return L.FfnDesc(rows=rows, width=width, dtype=dtype, activation=_ACT[act], ln_eps=1e-3, matmul=_MM[matmul], flags=0)


@pytest.mark.parametrize("W", sorted(MODES))
def test_ffn_supports_bf16_storage_at_every_width_and_mode(W, egt_lib):
    lib = L.load()
    for mm in MODES[W]:
        for act in ("elu", "relu"):
            for rows in (1, 17, 150 * 150 * 2 + 3):
                d = _ffn(rows, W, L.EGT_BF16, mm, act)
                assert lib.egt_ffn_supported(C.byref(d)) == 1, (W, mm, act, rows)
                nb = lib.egt_ffn_workspace_bytes(C.byref(d))
                assert nb > 0
                # the workspace holds fp32 operands and partials in both dtypes: same plan as the fp32 twin
                assert nb == lib.egt_ffn_workspace_bytes(C.byref(_ffn(rows, W, L.EGT_F32, mm, act)))
        assert lib.egt_ffn_supported(C.byref(_ffn(64, W, 5, mm))) == 0
        assert lib.egt_ffn_workspace_bytes(C.byref(_ffn(64, W, 5, mm))) == 0
    if W == 8:   # width 8 stays exact-fp32-products only
        for mm in ("bf16x3", "bf16"):
            assert lib.egt_ffn_supported(C.byref(_ffn(64, 8, L.EGT_BF16, mm))) == 0


def test_fp32_ffn_workspace_sizes_are_unchanged(egt_lib):
    """fp32 answers are pinned by tests/golden/op_workspace.json (test_op_workspace_cpu); a bf16 descriptor gets its fp32
    twin's size: the storage dtype changes the kernel instances, not the plan"""
    lib = L.load()
    gold = json.load(open(os.path.join(REPO, "tests", "golden", "op_workspace.json")))
    names = {"f32": "f32", "bf16x3": "bf16x3", "bf16": "bf16"}
    checked = 0
    for W in (16, 32, 48, 64):
        for mm in MODES[W]:
            for rows in (1, 100, 524288):
                key = f"ffn_W{W}_{names[mm]}_elu_rows{rows}"
                if key not in gold:
                    continue
                assert lib.egt_ffn_workspace_bytes(C.byref(_ffn(rows, W, L.EGT_F32, mm))) == gold[key], key
                assert lib.egt_ffn_workspace_bytes(C.byref(_ffn(rows, W, L.EGT_BF16, mm))) == gold[key], key
                checked += 1
    assert checked >= 12


def test_ffn_bf16_argument_errors_come_back_without_a_launch(egt_lib):
    lib = L.load()
    ps = L.FfnParams()
    d = _ffn(64, 8, L.EGT_BF16)
    assert lib.egt_ffn_fwd(C.byref(d), C.byref(ps), None, None, None, None) == L.EGT_E_NULL
    bad = _ffn(64, 8, 7)
    ws = (C.c_char * 64)()
    assert lib.egt_ffn_fwd(C.byref(bad), C.byref(ps), None, None, ws, None) == L.EGT_E_DTYPE
    assert lib.egt_ffn_bwd(C.byref(bad), C.byref(ps), None, None, None, C.byref(ps), ws, None) == L.EGT_E_DTYPE
    assert lib.egt_ffn_fwd(C.byref(_ffn(64, 24, L.EGT_BF16)), C.byref(ps), None, None, ws, None) == L.EGT_E_SHAPE


def _embed(dtype, De=8, K=4, V=0, F=0, B=2, N=9):
    from egt_amd.model import _embed_desc
    import torch
    d = _embed_desc(B, N, De, K, True, V, F, -1.0, torch.bfloat16 if dtype == L.EGT_BF16 else torch.float32)
    d.dtype = dtype
    return d


def test_edge_embed_supports_bf16_storage(egt_lib):
    lib = L.load()
    for De, K, V, F in ((8, 4, 0, 1), (64, 16, 4, 0), (16, 1, 7, 4), (48, 16, 5, 2)):
        b, f = _embed(L.EGT_BF16, De, K, V, F), _embed(L.EGT_F32, De, K, V, F)
        assert lib.egt_edge_embed_supported(C.byref(b)) == 1
        assert lib.egt_edge_embed_hops_bytes(C.byref(b)) == lib.egt_edge_embed_hops_bytes(C.byref(f)) > 0   # hop planes stay fp32
        assert lib.egt_edge_embed_workspace_bytes(C.byref(b)) == lib.egt_edge_embed_workspace_bytes(C.byref(f)) > 0
    for dt in (2, 5):
        d = _embed(dt)
        assert lib.egt_edge_embed_supported(C.byref(d)) == 0
        assert lib.egt_edge_embed_hops_bytes(C.byref(d)) == 0 and lib.egt_edge_embed_workspace_bytes(C.byref(d)) == 0
        assert lib.egt_edge_embed_fwd(C.byref(d), None, None, None, None, None, None, None, None, None) == L.EGT_E_DTYPE
        assert lib.egt_edge_embed_bwd(C.byref(d), None, None, None, None, None, None, None, None) == L.EGT_E_DTYPE
    assert lib.egt_edge_embed_fwd(C.byref(_embed(L.EGT_BF16)), None, None, None, None, None, None, None, None, None) == L.EGT_E_NULL


def test_make_config_takes_edge_dtype():
    from egt_amd import training as T
    assert T.make_config({}, "cifar10.svd").edge_dtype == "f32"
    assert T.make_config({"edge_dtype": "bf16"}, "cifar10.svd").edge_dtype == "bf16"
    for bad in ("fp16", "bfloat16", None, 1):
        with pytest.raises(ValueError, match="edge_dtype"):
            T.make_config({"edge_dtype": bad}, "cifar10.svd")


@pytest.mark.parametrize("scheme,path", [("zinc.svd", None), ("pattern.svd", None), ("cifar10.svd", None),
                                         ("cifar10.svd", "cifar10_100k_egt_spe.json"), ("zinc.eig", "zinc_100k_egt_epe.json")])
def test_model_config_is_unchanged_by_the_edge_dtype_key(scheme, path):
    """model_config() is the reference's: the project key reaches the model through get_model only"""
    from egt_amd import training as T
    user = json.load(open(os.path.join(REPO, "tests", "configs", path))) if path else {"scheme": scheme}
    scheme = user.get("scheme", scheme)
    base = T.model_config(T.make_config(dict(user), scheme))
    assert "edge_dtype" not in base
    assert T.model_config(T.make_config(dict(user, edge_dtype="bf16"), scheme)) == base
    s = T.import_scheme(scheme)(dict(user, edge_dtype="bf16"), model_factory=lambda mc: mc)
    assert s.get_model_config() == base
    assert s.model_kwargs() == dict(base, edge_dtype="bf16")


def test_models_refuse_an_unknown_edge_dtype(egt_lib):
    from egt_amd import Cifar10DCTransformer
    with pytest.raises(ValueError, match="edge_dtype"):
        Cifar10DCTransformer(model_width=32, model_height=1, upto_hop=4, edge_dtype="fp16")


@pytest.mark.parametrize("kw,why", [(dict(num_heads=4), "fused block"), (dict(scale_degree=True), "scale_degree"),
                                    (dict(attn_dropout=0.1), "attn_dropout")])
def test_bf16_model_refuses_what_it_cannot_run(kw, why, egt_lib):
    """bf16 edges run on the fused block + fused FFN only: an uncovered geometry is a ValueError at construction (never an
    fp32 fall-back, never a TypeError at the first step); the same model in fp32 still builds"""
    from egt_amd import Cifar10DCTransformer, ZincDCTransformer
    base = dict(model_width=32, model_height=2, upto_hop=4)
    base.update(kw)
    with pytest.raises(ValueError, match=why):
        Cifar10DCTransformer(edge_dtype="bf16", **base)
    Cifar10DCTransformer(**base)
    m = ZincDCTransformer(model_width=32, edge_width=64, model_height=1, upto_hop=4, edge_dtype="bf16")
    assert m.edge_dtype.is_floating_point and str(m.edge_dtype) == "torch.bfloat16"
