"""Distance objective without a GPU: the composed head against the fp64 restatement (distance_ref.py), the C-ABI
declarations against their ctypes mirrors, the reference's egt_spe_do configs (tests/golden/distance/) through the config
path, and the geometries the models keep refusing."""
import ctypes as C
import glob
import json
import os
import subprocess

import pytest
import torch

import distance_ref as DR
from util import assert_close, FWD, BWD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "distance", "*.json")))


@pytest.mark.parametrize("De,width,T,act,ln", [(48, 48, 3, "elu", True), (8, 64, 8, "relu", True), (16, 64, 3, "elu", False)])
def test_composed_head_matches_the_restatement(De, width, T, act, ln):
    from egt_amd.head import distance_head_composed, distance_target
    adj = DR.make_graphs(19)
    target = DR.ref_target(adj, T)
    assert torch.equal(distance_target(adj, T).long(), target)
    assert sorted(target.unique().tolist()) == list(range(T + 1))
    g = torch.Generator().manual_seed(3)
    e = torch.randn(3, 19, 19, De, generator=g) * 1.5 + 0.3
    s = torch.tensor([0.7, -1.3, 0.45])
    params = DR.head_params(De, width, T, ln)
    e64 = e.double().requires_grad_()
    p64 = tuple(None if p is None else p.double().requires_grad_() for p in params)
    ref = DR.ref_head(e64, target, p64, act)
    gref = torch.autograd.grad(ref, [e64] + [p for p in p64 if p is not None], s.double())
    e32 = e.clone().requires_grad_()
    p32 = tuple(None if p is None else p.clone().requires_grad_() for p in params)
    out = distance_head_composed(e32, target.to(torch.uint8), p32, act)
    got = torch.autograd.grad(out, [e32] + [p for p in p32 if p is not None], s)
    assert_close(out, ref, name="per_graph", **FWD)
    assert float(out[2].detach()) == 0.0, "the graph without edges has no loss"
    for n, a, r in zip(("d_e",) + (DR.HEAD_NAMES if ln else DR.HEAD_NAMES[2:]), got, gref):
        assert_close(a, r, name=n, **BWD)
    assert float(got[0][target == 0].abs().max()) == 0.0


def test_target_is_independent_of_padding_and_clips_always():
    """padded pairs have adjacency 0, hence target 0; a pair connected by k of the first T hop matrices has target k"""
    t = DR.ref_target(DR.make_graphs(19), 3)
    assert int(t[:, 16:, :].max()) == 0 and int(t[:, :, 16:].max()) == 0
    a = DR.lollipop(16, 19)
    h2 = torch.clamp(a @ a, 0, 1)
    h3 = torch.clamp(a @ h2, 0, 1)
    assert torch.equal(t[0].double(), (a + h2 + h3).double())


def test_header_protos_and_struct_layouts_agree(egt_lib, tmp_path):
    from egt_amd import _lib as L
    import re
    src = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("egt_distance_target", 6), ("egt_edge_head_supported", 1), ("egt_edge_head_workspace_bytes", 1),
                        ("egt_edge_head_fwd", 7), ("egt_edge_head_bwd", 9)):
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L._PROTOS[name][1]), name
        assert hasattr(egt_lib, name)
    assert re.search(r"#define EGT_EH_LAYERNORM (0x[0-9a-fA-F]+)", src).group(1) == hex(L.EH_LAYERNORM)
    assert re.search(r"#define EGT_ABI_VERSION (\d+)", src).group(1) == str(L.ABI_VERSION) == "4"
    pairs = [("egt_head_desc", L.HeadDesc), ("egt_head_params", L.HeadParams)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [f for f, _ in L.HeadParams._fields_] == [n.replace("/", "_") for n in DR.HEAD_NAMES], "the Keras order"


def test_descriptor_answers_without_a_launch(egt_lib):
    from egt_amd import _lib as L
    from egt_amd.head import head_desc
    sup = lambda d: egt_lib.egt_edge_head_supported(C.byref(d))
    for De in (8, 16, 32, 48, 64):
        for m0, m1 in ((24, 12), (32, 16)):
            for dt in (torch.float32, torch.bfloat16):
                assert sup(head_desc(4, 37, De, m0, m1, 4, dtype=dt)) == 1
    assert sup(head_desc(4, 37, 64, 32, 16, 16, "relu")) == 1 and sup(head_desc(4, 37, 64, 32, 16, 2, layernorm=False)) == 1
    for bad in (head_desc(4, 37, 24, 32, 16, 4), head_desc(4, 37, 64, 8, 4, 4), head_desc(4, 37, 64, 32, 12, 4),
                head_desc(4, 37, 64, 32, 16, 17), head_desc(4, 37, 64, 32, 16, 1), head_desc(70000, 200, 64, 32, 16, 4)):
        assert sup(bad) == 0 and egt_lib.egt_edge_head_workspace_bytes(C.byref(bad)) == 0
    d = head_desc(4, 37, 64, 32, 16, 4); d.activation = L.ACT_LRELU
    assert sup(d) == 0
    d = head_desc(4, 37, 64, 32, 16, 4); d.flags = 0x2
    prm = L.HeadParams()
    assert egt_lib.egt_edge_head_fwd(C.byref(d), C.byref(prm), None, None, None, None, None) == L.EGT_E_FLAGS
    d = head_desc(4, 37, 64, 32, 16, 4)
    assert egt_lib.egt_edge_head_fwd(C.byref(d), C.byref(prm), None, None, None, None, None) == L.EGT_E_NULL
    assert egt_lib.egt_edge_head_fwd(C.byref(d), None, None, None, None, None, None) == L.EGT_E_NULL
    d.dtype = 7
    assert egt_lib.egt_edge_head_fwd(C.byref(d), C.byref(prm), None, None, None, None, None) == L.EGT_E_DTYPE
    assert egt_lib.egt_distance_target(None, 2, 19, 3, None, None) == L.EGT_E_NULL
    assert egt_lib.egt_distance_target(None, 2, 500, 3, None, None) == L.EGT_E_SHAPE
    ws = egt_lib.egt_edge_head_workspace_bytes
    assert ws(C.byref(head_desc(128, 37, 64, 32, 16, 4))) > ws(C.byref(head_desc(128, 37, 8, 32, 16, 4))) > 0


def test_three_fixture_configs_are_present():
    assert [os.path.basename(p) for p in CONFIGS] == ["cifar10_100k_egt_spe_do.json", "zinc_100k_egt_spe_do.json",
                                                      "zinc_500k_egt_spe_do.json"]


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(p)[:-5] for p in CONFIGS])
def test_reference_spe_do_configs_load(path, egt_lib):
    from egt_amd import training as T
    cfg = json.load(open(path))
    c = T.make_config(cfg)
    mc = T.model_config(c)
    assert mc["distance_loss"] == cfg["distance_loss"] > 0 and mc["distance_target"] == cfg["distance_target"] == 3
    s = T.import_scheme(cfg["scheme"])(cfg)
    assert "distance_loss" in s.get_metrics() and "distance_loss" in s.metric_keys()
    model = s.get_model()
    names = set(model.keras_named_parameters())
    assert set(DR.HEAD_NAMES) <= names
    Ly = cfg["model_height"]
    for k in (f"dense_edge_r_{Ly - 1:0>2d}/kernel", f"fnn_lr1_edge_{Ly - 1:0>2d}/kernel", f"norm_fnn_edge_{Ly - 1:0>2d}/gamma"):
        assert k in names, f"{k}: the last layer's edge side is live with the objective on"
    assert model._dead_edge_params() == [] and len(model.trainable_parameters()) == len(names)
    assert model.dist_head.num_classes == 4
    assert tuple(model.dist_head.distance_target.kernel.shape) == (round(.25 * cfg["model_width"]), 4)
    # the objective off: the model and its parameter names are what they were
    off = T.import_scheme(cfg["scheme"])(dict(cfg, distance_loss=0.)).get_model()
    assert off.dist_head is None and not (set(DR.HEAD_NAMES) & set(off.keras_named_parameters()))
    assert "distance_loss" not in T.import_scheme(cfg["scheme"])(dict(cfg, distance_loss=0.)).get_metrics()


def test_unsupported_geometries_stay_refused(egt_lib):
    from egt_amd import ZincDCTransformer, Cifar10DCTransformer
    ok = dict(model_width=48, edge_width=48, model_height=2, distance_loss=.05, distance_target=3)
    assert ZincDCTransformer(**ok).dist_head is not None
    for change in (dict(model_width=16, edge_width=16), dict(mlp_layers=[.5]), dict(distance_target=16), dict(distance_target=0),
                   dict(edge_channel_type="bias", model_width=64, edge_width=8)):
        with pytest.raises(NotImplementedError, match="covers the shipped configs; not built"):
            ZincDCTransformer(**dict(ok, **change))
    with pytest.raises(NotImplementedError, match="covers the shipped configs; not built"):
        Cifar10DCTransformer(model_width=32, edge_width=8, model_height=2, distance_loss=.0005, distance_target=3)
    assert Cifar10DCTransformer(model_width=64, edge_width=8, model_height=2, distance_loss=.0005, distance_target=3,
                                edge_dtype="bf16").dist_head is not None


def test_cpu_model_has_no_silent_fallback(egt_lib):
    from egt_amd import DistanceHead
    head = DistanceHead(48, 48, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        head(torch.zeros(1, 4, 4, 48), torch.zeros(1, 4, 4, dtype=torch.uint8))
