"""Fused graph-level readout head on the GPU (egt_graph_head_fwd / egt_graph_head_bwd): stats, predictions and every gradient
against the fp64 oracle (graph_head_ref.py) and against the composed head on the GPU; the contract's exact zeros, padding,
determinism, homogeneity; ill-conditioned inputs; the models' graph_loss and the schemes on the fused route."""
import os
import subprocess
import sys

import pytest
import torch

import graph_head_ref as GR
import virtual_nodes_ref as VR
from util import assert_close, bf16_stack_tol, FWD, BWD

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fused(c, gpu, **kw):
    from egt_amd.graph_head import graph_head_loss
    return GR.run(graph_head_loss, c, gpu, **kw)


def _check(got, ref, c, tag):
    assert_close(got["stats"][0], ref["stats"][0], name=f"loss sum vs {tag}", **FWD)
    assert got["stats"][1:].tolist() == ref["stats"][1:].tolist(), f"hits and count vs {tag}: exact"
    assert_close(got["pred"], ref["pred"], name=f"pred vs {tag}", **FWD)
    assert_close(got["d_h"], ref["d_h"], name=f"d_h vs {tag}", **BWD)
    for n, a, r in zip(GR.grad_names(c), got["grads"], ref["grads"]):
        assert_close(a, r, name=f"d {n} vs {tag}", **BWD)


@pytest.mark.parametrize("cid", list(GR.CASES))
def test_forward_backward(cid, gpu, egt_lib):
    from egt_amd.graph_head import graph_head_composed
    c, ref = GR.reference(cid)
    assert ref["fair"] >= 1e-3
    got, st = _fused(c, gpu)
    assert type(st.grad_fn).__name__ == "_FusedGraphHeadBackward"
    comp, _ = GR.run(graph_head_composed, c, gpu)
    _check(got, ref, c, "fp64")
    _check(got, comp, c, "composed")
    assert float(got["stats"][2]) == (c["B"] * c["C"] if c["loss"] == "mae" else c["B"])
    zero = GR.zero_rows(c).to(gpu)
    if bool(zero.any()):
        assert float(got["d_h"][zero].abs().max()) == 0.0, "exact zeros where the contract says so"
    assert bool((got["d_h"][~zero].abs().amax(-1) > 0).all()), "every other row has a gradient"


@pytest.mark.parametrize("cid", GR.RECIPE_CASES)
@pytest.mark.parametrize("recipe", GR.RECIPES)
def test_ill_conditioned_inputs(cid, recipe, gpu, egt_lib):
    c, ref = GR.reference(cid, recipe)
    assert ref["fair"] >= 1e-3
    got, _ = _fused(c, gpu)
    _check(got, ref, c, f"fp64 ({recipe})")


@pytest.mark.parametrize("cid", ["w64_mae_n19", "w64_xent_n150", "w64_mae_nv1"])
def test_padded_rows_change_no_bit(cid, gpu, egt_lib):
    """the rows the readout does not use (masked ones; with virtual nodes every row behind them) filled with the value 32"""
    c, _ = GR.reference(cid)
    a, _ = _fused(c, gpu)
    h = c["h"].clone()
    h[GR.zero_rows(c)] = 32.0
    assert not torch.equal(h, c["h"])
    b, _ = _fused(c, gpu, h=h)
    for k in ("stats", "pred", "d_h"):
        assert torch.equal(a[k], b[k]), k
    for p, q in zip(a["grads"], b["grads"]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("cid", ["w64_mae_n19", "w64_mae_b70", "w64_xent_nv2"])
def test_two_calls_are_bitwise_equal(cid, gpu, egt_lib):
    c, _ = GR.reference(cid)
    a, _ = _fused(c, gpu)
    b, _ = _fused(c, gpu)
    for k in ("stats", "pred", "d_h"):
        assert torch.equal(a[k], b[k]), k
    for p, q in zip(a["grads"], b["grads"]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("cid", ["w64_mae_n19", "w64_xent_n19"])
def test_upstream_gradient_scales_the_gradients(cid, gpu, egt_lib):
    """the upstream gradient is read on the device; a power of two scales every gradient exactly"""
    c, _ = GR.reference(cid)
    one, _ = _fused(c, gpu, up=1.0)
    for f in (4.0, 0.25):
        other, _ = _fused(c, gpu, up=f)
        assert torch.equal(one["stats"], other["stats"]) and torch.equal(one["pred"], other["pred"])
        assert torch.equal(one["d_h"] * f, other["d_h"]) and float(one["d_h"].abs().max()) > 0
        for p, q in zip(one["grads"], other["grads"]):
            assert torch.equal(p * f, q)


def test_gradients_land_in_bound_sinks(gpu, egt_lib):
    """FlatGradAllReduce(direct=True): the eight parameter gradients are written into their views of the flat buffer"""
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.graph_head import graph_head_loss
    c, _ = GR.reference("w48_mae_n37")
    want, _ = _fused(c, gpu)
    ps = tuple(torch.nn.Parameter(p.to(gpu)) for p in c["params"])
    ar = FlatGradAllReduce(list(ps), direct=True)
    ar.flat.fill_(float("nan"))                  # a sink is overwritten, not accumulated into
    ptrs = [p.grad.data_ptr() for p in ps]
    h = c["h"].to(gpu).requires_grad_()
    st, _ = graph_head_loss(h, c["target"].to(gpu), c["mask"].to(gpu), ps, c["loss"], c["nv"], c["act"])
    (st[0] * GR.S_UP).backward()
    assert [p.grad.data_ptr() for p in ps] == ptrs, "the gradients are the views of the flat buffer"
    for p, g in zip(ps, want["grads"]):
        assert torch.equal(p.grad, g)
    assert torch.equal(h.grad, want["d_h"])


# ------------------------------------------------------------------------------------------- models and schemes -----
def _prof_names(lib):
    import ctypes as C
    buf = C.create_string_buffer(1 << 16)
    lib.egt_prof_names(buf, len(buf))
    return buf.value.decode()


def _model_case(kind, nv, edge_dtype, gpu, Dh=64):
    from egt_amd import ZincDCTransformer, Cifar10DCTransformer
    from oracle import egt_model_oracle as MO
    De = 8 if kind == "cifar10" else 64
    cfg = dict(model_width=Dh, edge_width=De, model_height=2, upto_hop=4, num_targets=10 if kind == "cifar10" else 1)
    g = torch.Generator().manual_seed(1000 + nv + len(kind))
    counts = [19, 7, 12]
    inp = VR.graphs(kind, 3, 19, counts, g)
    if nv:
        params = VR.init_params(kind, cfg, nv, g)
    else:
        c2 = dict(cfg, float_node_features=5, float_edge_features=1) if kind == "cifar10" else cfg
        params = MO.init_zinc_params(c2, dtype=torch.float32, generator=g)
        if kind == "cifar10":
            params.pop("node_emb.embeddings"); params.pop("fm_emb.embeddings")
    cls = Cifar10DCTransformer if kind == "cifar10" else ZincDCTransformer
    model = cls(model_width=Dh, edge_width=De, model_height=2, upto_hop=4, num_virtual_nodes=nv, random_mask_prob=0.0,
                edge_dtype=edge_dtype).to(gpu).eval()
    with torch.no_grad():
        for k, v in params.items():
            prm = VR.module_param(model, k)
            if prm is not None:
                prm.copy_(v)
    return model, inp, params, cfg


def _oracle(kind, nv, inp, params, cfg):
    from oracle import egt_model_oracle as MO
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    if nv:
        yo = VR.forward(kind, inp, p64, cfg, nv)
    elif kind == "cifar10":
        yo = MO.cifar10_forward(inp["node_features"], inp["feature_matrix"], inp["graph_matrix"], p64,
                                dict(cfg, float_node_features=5, float_edge_features=1))
    else:
        yo = MO.zinc_forward(inp["node_features"], inp["feature_matrix"], inp["graph_matrix"], p64, cfg)
    loss = MO.sparse_xent_loss(yo, inp["target"]) if kind == "cifar10" else MO.mae_loss(yo, inp["target"].double())
    return yo.detach(), loss, dict(zip(p64, torch.autograd.grad(loss, list(p64.values()), allow_unused=True)))


@pytest.mark.parametrize("kind,nv,edge_dtype", [("zinc", 0, "f32"), ("zinc", 1, "f32"), ("cifar10", 0, "f32"), ("cifar10", 0, "bf16")])
def test_graph_loss_takes_the_fused_route_and_matches_the_model_oracle(kind, nv, edge_dtype, gpu, egt_lib):
    model, inp, params, cfg = _model_case(kind, nv, edge_dtype, gpu)
    dev = lambda k: inp[k].to(gpu)
    egt_lib.egt_prof_enable(2)
    try:
        loss, stats, pred, aux = model.graph_loss(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"), dev("target"))
        loss.backward()
        torch.cuda.synchronize()
        names = _prof_names(egt_lib)
    finally:
        egt_lib.egt_prof_enable(0)
    assert aux == {} and type(stats.grad_fn).__name__ == "_FusedGraphHeadBackward"
    assert model.graph_head_fused(torch.empty(3, nv + 19, 64, device=gpu))
    assert "k_graph_head_fwd" in names and "k_graph_head_bwd" in names
    yo, loss_o, gro = _oracle(kind, nv, inp, params, cfg)
    tol, ptol = (dict(rtol=2e-4, arel=5e-5), BWD) if edge_dtype == "f32" else \
        (bf16_stack_tol(2), dict(bf16_stack_tol(2, params=True), zero_atol=2e-4))
    assert_close(pred, yo, name="pred", **tol)
    assert_close(loss.reshape(1), loss_o.reshape(1), name="loss", **tol)
    B = 3
    assert float(stats[2].detach()) == (B if kind == "cifar10" else B * 1)
    if kind == "cifar10":
        assert float(stats[1].detach()) == float((yo.argmax(-1) == inp["target"]).sum())
    live = {id(v) for v in model.keras_named_parameters().values()}
    checked = 0
    for k, gref in gro.items():
        prm = VR.module_param(model, k)
        if prm is None or id(prm) not in live or gref is None:
            continue
        assert_close(prm.grad, gref, name=k, **ptol); checked += 1
    assert checked == len(live)
    # forward is unchanged and agrees with the op's predictions
    with torch.no_grad():
        y = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
    assert_close(pred, y, name="pred vs forward", **FWD)


def test_uncovered_geometry_raises_and_the_models_fall_back(gpu, egt_lib):
    from egt_amd.graph_head import graph_head_composed, graph_head_loss
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(gpu)
    W = 32
    params = (1 + 0.1 * rn(W), 0.1 * rn(W), rn(W, 16) * 0.2, rn(16) * 0.1, rn(16, 8) * 0.3, rn(8) * 0.1, rn(8, 1) * 0.3, rn(1) * 0.1)
    h, mask, t = rn(3, 19, W), torch.ones(3, 19, dtype=torch.bool, device=gpu), rn(3, 1)
    with pytest.raises(ValueError, match="graph head kernel covers"):
        graph_head_loss(h, t, mask, params, "mae", 0, "elu")
    with pytest.raises(TypeError):
        c, _ = GR.reference("w64_xent_n19")
        graph_head_loss(c["h"].to(gpu), c["target"].float().to(gpu), c["mask"].to(gpu), tuple(p.to(gpu) for p in c["params"]), "xent")
    model, inp, _, _ = _model_case("zinc", 0, "f32", gpu, Dh=32)
    assert not model.graph_head_fused(torch.empty(3, 19, 32, device=gpu))
    dev = lambda k: inp[k].to(gpu)
    loss, stats, pred, _ = model.graph_loss(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"), dev("target"))
    assert type(stats.grad_fn).__name__ != "_FusedGraphHeadBackward"
    from egt_amd import mae_loss
    y = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
    assert_close(loss, mae_loss(y, dev("target")), name="composed loss", rtol=1e-5, arel=1e-6)
    assert_close(pred, y, name="composed pred", rtol=1e-5, arel=1e-6)


_CHILD = r"""
import sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import graph_head_ref as GR, virtual_nodes_ref as VR
from egt_amd import ZincDCTransformer
from egt_amd.graph_head import graph_head_composed, graph_head_disabled
gpu = torch.device("cuda:0")
torch.manual_seed(11)
model = ZincDCTransformer(model_width=64, edge_width=64, model_height=1, upto_hop=4, random_mask_prob=0.0).to(gpu).eval()
inp = VR.graphs("zinc", 3, 19, [19, 7, 12], torch.Generator().manual_seed(3))
d = lambda k: inp[k].to(gpu)
assert graph_head_disabled() and not model.graph_head_fused(torch.empty(3, 19, 64, device=gpu))
loss, stats, pred, _ = model.graph_loss(d("node_features"), d("feature_matrix"), d("graph_matrix"), d("target"))
assert type(stats.grad_fn).__name__ != "_FusedGraphHeadBackward"
loss.backward()
h, e, mask = model.embeddings(d("node_features"), d("feature_matrix"), d("graph_matrix"))
h, e = model.layers(h, e, mask, None, skip_last_edge_ffn=True)
st2, pred2 = graph_head_composed(h, d("target"), mask, model.graph_head_params(), "mae", 0, "elu")
assert torch.equal(st2.detach(), stats.detach()) and torch.equal(pred2.detach(), pred)
print("CHILD-OK", float(loss))
"""


def test_switch_keeps_the_composed_head(gpu, egt_lib, tmp_path):
    """EGT_NO_GRAPH_HEAD=1 is read once per process: a child process"""
    src = tmp_path / "child.py"
    src.write_text(_CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests")))
    r = subprocess.run([sys.executable, str(src)], env=dict(os.environ, EGT_NO_GRAPH_HEAD="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, r.stdout + r.stderr


def _zinc_run(tag, graph, tmp_path, gpu, epochs=3):
    import egt_amd.training as T
    torch.manual_seed(0)
    cfg = dict(scheme="zinc.svd", model_width=64, edge_width=64, batch_size=8, model_name=tag, num_epochs=epochs, initial_lr=2e-3,
               use_svd=False, model_height=2, upto_hop=4, random_mask_prob=0.0, use_hipgraph=graph, save_path=str(tmp_path / tag))
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
    s.execute_training(T.SyntheticZinc(32, 8, seed=1, pad_multiple=1), T.SyntheticZinc(16, 8, seed=2, pad_multiple=1))
    return s


def test_use_hipgraph_reproduces_the_eager_training_run(tmp_path, gpu, egt_lib):
    eager, graphed = _zinc_run("e", False, tmp_path, gpu), _zinc_run("g", True, tmp_path, gpu)
    assert eager.model.graph_head_fused(torch.empty(8, 20, 64, device=gpu))
    assert len(graphed._graphs) >= 2
    assert [h["loss"] for h in graphed.history] == [h["loss"] for h in eager.history] and len(eager.history) == 3
    assert [h["val_mae"] for h in graphed.history] == [h["val_mae"] for h in eager.history]
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)


def test_evaluate_returns_the_composed_mae(tmp_path, gpu, egt_lib):
    import egt_amd.training as T
    s = _zinc_run("v", False, tmp_path, gpu, epochs=1)
    val = list(T.SyntheticZinc(16, 8, seed=2, pad_multiple=1))
    got = s.evaluate(val)["mae"]
    s.model.eval()
    sabs, n = 0.0, 0
    with torch.no_grad():
        for b in val:
            y = s.model(b["node_features"].to(gpu), b["feature_matrix"].to(gpu), b["graph_matrix"].to(gpu))
            sabs += float((y - b["target"].to(gpu)).abs().sum()); n += b["target"].numel()
    assert_close(torch.tensor([float(got)]), torch.tensor([sabs / n]), name="val mae", **FWD)
