"""Virtual nodes without a GPU: the C-ABI of the bordered edge embedding (symbols, ABI version, coverage answers), what the
models build and keep refusing, the schemes' config path, and the fp64 restatement (virtual_nodes_ref.py) against the index
formulas of the border."""
import ctypes as C
import os
import re

import pytest
import torch

import virtual_nodes_ref as VR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VN_SYMBOLS = {"egt_edge_embed_vn_supported": 2, "egt_edge_embed_vn_workspace_bytes": 2, "egt_edge_embed_vn_fwd": 12,
              "egt_edge_embed_vn_bwd": 11}


def test_library_exports_the_vn_entry_points_and_keeps_abi_4(egt_lib):
    from egt_amd import _lib as L
    src = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in VN_SYMBOLS.items():
        assert hasattr(egt_lib, name), name
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L._PROTOS[name][1]), name
    assert re.search(r"#define EGT_ABI_VERSION (\d+)", src).group(1) == str(L.ABI_VERSION) == "4"
    assert egt_lib.egt_abi_version() == 4


def test_vn_supported_answers_without_a_launch(egt_lib):
    from egt_amd.model import _embed_desc
    sup = lambda d, nv: egt_lib.egt_edge_embed_vn_supported(C.byref(d), nv)
    for De in (8, 64):
        for dt in (torch.float32, torch.bfloat16):
            d = _embed_desc(4, 37, De, 16, True, 4, dtype=dt)
            assert sup(d, 1) == 1 and sup(d, 16) == 1
            assert sup(d, 0) == 0 and sup(d, 17) == 0 and sup(d, -1) == 0
            ws, ws0 = egt_lib.egt_edge_embed_vn_workspace_bytes, egt_lib.egt_edge_embed_workspace_bytes(C.byref(d))
            assert ws(C.byref(d), 2) == ws0 + 4 * 2 * De * 4 and ws(C.byref(d), 0) == 0 and ws(C.byref(d), 17) == 0
    bad = _embed_desc(4, 37, 6, 16, True, 4)
    assert egt_lib.egt_edge_embed_supported(C.byref(bad)) == 0 and sup(bad, 1) == 0
    assert sup(_embed_desc(4, 37, 8, 16, True, 4, num_float_features=1), 3) == 1


def test_vn_entry_points_check_their_arguments(egt_lib):
    from egt_amd import _lib as L
    from egt_amd.model import _embed_desc
    d = _embed_desc(2, 19, 8, 4, True, 4)
    nul = [None] * 10
    assert egt_lib.egt_edge_embed_vn_fwd(C.byref(d), 1, *nul) == L.EGT_E_NULL
    assert egt_lib.egt_edge_embed_vn_fwd(C.byref(d), 0, *nul) == L.EGT_E_SHAPE
    assert egt_lib.egt_edge_embed_vn_fwd(C.byref(d), 17, *nul) == L.EGT_E_SHAPE
    assert egt_lib.egt_edge_embed_vn_bwd(C.byref(d), 1, *nul[:9]) == L.EGT_E_NULL
    assert egt_lib.egt_edge_embed_vn_bwd(C.byref(d), 17, *nul[:9]) == L.EGT_E_SHAPE


def test_zinc_model_with_virtual_nodes_builds_on_the_cpu():
    from egt_amd import ZincDCTransformer
    m = ZincDCTransformer(model_width=16, edge_width=16, model_height=1, num_virtual_nodes=2)
    named = m.keras_named_parameters()
    for k in ("virtual_node_embedding/virtual_node_embeddings", "virtual_edge_embedding/virtual_edge_embeddings"):
        assert tuple(named[k].shape) == (2, 16), k
        assert float(named[k].detach().abs().max()) <= 0.05                      # Keras 'uniform'
        assert any(p is named[k] for p in m.trainable_parameters()), k
    assert tuple(named["mlp_out_0/kernel"].shape) == (32, 8)
    assert [b.mha.num_virtual_nodes for b in m.layers.blocks] == [0]
    ms = ZincDCTransformer(model_width=16, edge_width=16, model_height=1, num_virtual_nodes=2, scale_degree=True)
    assert [b.mha.num_virtual_nodes for b in ms.layers.blocks] == [2]
    m0 = ZincDCTransformer(model_width=16, edge_width=16, model_height=1)
    assert not any(k.startswith("virtual_") for k in m0.keras_named_parameters())
    assert tuple(m0.keras_named_parameters()["mlp_out_0/kernel"].shape) == (16, 8)


def test_schemes_build_the_virtual_node_models(tmp_path):
    from egt_amd import training as T
    from egt_amd import ZincDCTransformer, Cifar10DCTransformer
    small = dict(model_width=16, edge_width=16, model_height=1, num_virtual_nodes=1, save_path=str(tmp_path / "run"))
    for cls, scheme, mcls in ((T.ZincSVDScheme, "zinc.svd", ZincDCTransformer), (T.Cifar10SVDScheme, "cifar10.svd", Cifar10DCTransformer)):
        s = cls(dict(small, scheme=scheme, model_name="v"))
        assert s.get_model_config()["num_virtual_nodes"] == 1
        model = s.get_model()
        assert type(model) is mcls and model.num_virtual_nodes == 1
        named = model.keras_named_parameters()
        assert tuple(named["virtual_node_embedding/virtual_node_embeddings"].shape) == (1, 16)
        assert tuple(named["virtual_edge_embedding/virtual_edge_embeddings"].shape) == (1, 16)
        assert tuple(named["mlp_out_0/kernel"].shape) == (16, 8)


def test_models_that_keep_refusing_virtual_nodes():
    from egt_amd import (ZincDCTransformer, Cifar10DCTransformer, PatternDCTransformer, ClusterDCTransformer,
                         MnistDCTransformer)
    small = dict(model_width=16, model_height=1)
    for cls in (PatternDCTransformer, ClusterDCTransformer, MnistDCTransformer):
        with pytest.raises(NotImplementedError, match="num_virtual_nodes"):
            cls(num_virtual_nodes=1, **small)
        cls(num_virtual_nodes=0, **small)
    for cls in (ZincDCTransformer, Cifar10DCTransformer):
        with pytest.raises(NotImplementedError, match="num_virtual_nodes=17"):
            cls(num_virtual_nodes=17, **small)
    with pytest.raises(NotImplementedError, match=r"distance_loss.*num_virtual_nodes"):
        ZincDCTransformer(model_width=64, edge_width=64, model_height=1, distance_loss=0.5, num_virtual_nodes=1)


@pytest.mark.parametrize("nv,N,De", [(1, 5, 4), (3, 4, 8)])
def test_restatement_agrees_with_the_index_formulas(nv, N, De):
    g = torch.Generator().manual_seed(nv * 10 + N)
    e = torch.randn(2, N, N, De, generator=g, dtype=torch.float64)
    emb = torch.randn(nv, De, generator=g, dtype=torch.float64)
    out = VR.virtual_edge_embedding(e, emb)
    assert out.shape == (2, nv + N, nv + N, De)
    assert torch.equal(out, VR.bordered_by_index(e, emb))
    assert torch.equal(out[:, nv:, nv:], e) and torch.equal(out[1, 0, nv + N - 1], emb[0]) and torch.equal(out[0, nv + 1, nv - 1], emb[nv - 1])
    # the gradient of the table under the formula of the kernel's border pass
    emb_g = emb.clone().requires_grad_()
    de = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (dv,) = torch.autograd.grad(VR.virtual_edge_embedding(e, emb_g), [emb_g], de)
    want = de[:, :nv, nv:].sum(dim=(0, 2)) + de[:, nv:, :nv].sum(dim=(0, 1)) \
        + 0.5 * (de[:, :nv, :nv].sum(dim=(0, 2)) + de[:, :nv, :nv].sum(dim=(0, 1)))
    assert torch.allclose(dv, want, rtol=1e-12, atol=1e-12)
    h = torch.randn(2, N, 6, generator=g, dtype=torch.float64)
    hv = VR.virtual_node_embedding(h, emb[:, :6] if De >= 6 else torch.ones(nv, 6, dtype=torch.float64))
    assert hv.shape == (2, nv + N, 6) and torch.equal(hv[:, nv:], h) and torch.equal(VR.get_virtual_nodes(hv, nv), hv[:, :nv])
