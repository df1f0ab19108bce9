"""GPU tests of the node-input embedding (egt_node_embed_fwd / _bwd through egt_amd.node_embed): the case table of
tests/node_embed_cases.py against the fp64 oracle under util.FWD / util.BWD, the mask bit for bit against egt_amd.masks,
exactness where the result is a copy, the models' routing, the EGT_NO_NODE_EMBED switch and a captured training step."""
import os
import subprocess
import sys

import pytest
import torch

import node_embed_cases as NC
from util import BWD, FWD, assert_close

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks_mask(c, gpu):
    from egt_amd.masks import node_mask_from_features, node_mask_from_masking
    f = c["features"].to(gpu)
    return node_mask_from_masking(f, -1.0, c["nv"]) if f.dtype.is_floating_point else node_mask_from_features(f, c["nv"])


@pytest.mark.parametrize("signs", [True, False], ids=["signs", "nosigns"])
@pytest.mark.parametrize("name", list(NC.CASES))
def test_forward_backward(name, signs, gpu, egt_lib):
    from egt_amd.node_embed import node_embed
    c = NC.make(name)
    h_ref, mask_ref, g_ref, gpos_ref = NC.oracle(c, signs)
    a, p = NC.args(c, torch.float32, gpu, signs=signs)
    h, mask = node_embed(*a)
    assert type(h.grad_fn).__name__ == "_FusedNodeEmbedBackward"
    assert mask.dtype == torch.bool and not mask.requires_grad
    assert torch.equal(mask, _masks_mask(c, gpu)) and torch.equal(mask.cpu(), mask_ref)
    assert_close(h, h_ref, name=f"{name}: h", **FWD)
    for up, ref in (("d_h", g_ref), ("d_h_pos", gpos_ref)):     # the one-sided upstream: a dropped partial sum cannot cancel
        got = NC.grads(h, p, c[up])
        assert set(got) == set(ref)
        for k in ref:
            assert_close(got[k], ref[k], name=f"{name}: d {k} ({up})", **BWD)


def test_plain_lookup_is_the_table_row_bit_for_bit(gpu, egt_lib):
    from egt_amd.node_embed import node_embed
    c = NC.make("lookup")
    a, p = NC.args(c, torch.float32, gpu, leaf=False)
    h, _ = node_embed(*a)
    assert torch.equal(h, p["node_emb"][(c["features"].to(gpu) + 1).long()])


@pytest.mark.parametrize("name", ["w16_nv2", "w32_nv16", "empty_n65_vn1_svd", "float5_svd_nv1"])
def test_virtual_rows_are_the_embedding_bit_for_bit(name, gpu, egt_lib):
    from egt_amd.node_embed import node_embed
    c = NC.make(name)
    a, p = NC.args(c, torch.float32, gpu, leaf=False)
    h, mask = node_embed(*a)
    nv = c["nv"]
    assert torch.equal(h[:, :nv], p["virtual_node_emb"][None].expand(c["B"], -1, -1)) and mask[:, :nv].all()


@pytest.mark.parametrize("name", ["b37_n40_svd_vn1", "float5_svd_nv1", "cluster_eig20"])
def test_two_backward_runs_are_bitwise_equal(name, gpu, egt_lib):
    from egt_amd.node_embed import node_embed
    c = NC.make(name)
    runs = []
    for _ in range(2):
        a, p = NC.args(c, torch.float32, gpu)
        h, _ = node_embed(*a)
        runs.append((h.detach(), NC.grads(h, p, c["d_h"])))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_pe_input_is_read_through_its_strides_and_sign_stride(gpu, egt_lib):
    """the encoding input is wider than what is used (sel of T) and the sign sample wider than sel (the untransformed
    encoding's padded draw): values past sel change nothing"""
    from egt_amd.node_embed import node_embed
    for name in ("empty_n65_vn1_svd", "svd_notransform", "w48_eig"):
        c = NC.make(name)
        a, _ = NC.args(c, torch.float32, gpu, leaf=False)
        h0, _ = node_embed(*a)
        a = list(a)
        sel = a[5]
        pe2 = a[3].clone()
        pe2[:, :, sel:] = 1e30
        sg2 = a[7].clone()
        sg2[:, :, sel:] = 1e30
        h1, _ = node_embed(a[0], a[1], a[2], pe2, a[4], sel, a[6], sg2, a[8], a[9])
        assert torch.equal(h0, h1), name


def test_gradients_land_in_bound_sinks(gpu, egt_lib):
    """a parameter whose .grad is a view of a flat buffer opened for direct writes receives its gradient there (fused.grad_sinks)"""
    from egt_amd.node_embed import node_embed
    c = NC.make("float5_svd_nv1")
    a, p = NC.args(c, torch.float32, gpu)
    h, _ = node_embed(*a)
    want = NC.grads(h, p, c["d_h"])
    a, p = NC.args(c, torch.float32, gpu)
    live = [k for k in NC.PARAMS if p[k] is not None]
    flat = torch.full((sum(p[k].numel() for k in live) + 3 * len(live),), float("nan"), device=gpu)
    off = 1                                                  # views at 4-byte alignment, as a flat gradient buffer gives them
    for k in live:
        p[k].grad = flat[off:off + p[k].numel()].view(p[k].shape)
        p[k]._egt_direct_grad = True
        off += p[k].numel() + 3
    h, _ = node_embed(a[0], p["node_emb"], p["node_emb_bias"], a[3], a[4], a[5], (p["pe_kernel"], p["pe_bias"]), a[7],
                      p["virtual_node_emb"], a[9])
    (h * c["d_h"].to(gpu)).sum().backward()
    for k in live:
        assert p[k].grad.data_ptr() >= flat.data_ptr() and torch.equal(p[k].grad, want[k]), k


def test_uncovered_geometry_raises(gpu, egt_lib):
    from egt_amd.node_embed import node_embed
    feat = torch.zeros(2, 5, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="node embedding kernel covers"):
        node_embed(feat, torch.zeros(29, 80, device=gpu))
    with pytest.raises(ValueError, match="node embedding kernel covers"):
        node_embed(feat, torch.zeros(33, 64, device=gpu))
    with pytest.raises(RuntimeError, match="no CPU path"):
        node_embed(feat.cpu(), torch.zeros(29, 64))


# ------------------------------------------------------------------------------------------------------ models -----
@pytest.mark.parametrize("which", list(NC.MODEL_RUNS))
def test_models_reach_the_kernels(which, gpu, egt_lib):
    """the kernels run inside the step, and the node segment itself launches no embedding / addmm op (nor their backward)"""
    r = NC.model_run(which, gpu, egt_lib)
    for k in ("k_node_embed_fwd", "k_node_embed_bwd", "k_node_embed_finish"):
        assert k in r["kernels"], (k, r["kernels"])
    assert torch.isfinite(r["loss"]) and all(torch.isfinite(g).all() for g in r["grads"].values())
    model, b = r["model"], r["batch"]
    model.zero_grad()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        h, mask = model.node_input(b["node_features"], r["pe"].get("singular_vectors"), r["pe"].get("eigen_vectors"))
        h.sum().backward()
        torch.cuda.synchronize()
    assert type(h.grad_fn).__name__ == "_FusedNodeEmbedBackward"
    ops = {e.key for e in prof.key_averages()}
    banned = [o for o in ops if any(s in o for s in ("embedding", "addmm", "aten::mm", "aten::cat", "aten::matmul"))]
    assert not banned, banned
    # and it is what the composed methods give
    model.eval()
    with torch.no_grad():
        h1, mask1 = model.node_input(b["node_features"], r["pe"].get("singular_vectors"), r["pe"].get("eigen_vectors"))
        h0, m0 = model._node_embedding(b["node_features"])
        h0 = model.with_virtual_nodes(model.positional(h0, r["pe"].get("singular_vectors"), r["pe"].get("eigen_vectors")))
    assert torch.equal(mask1, m0)
    assert_close(h1, h0.double(), name=f"{which}: fused vs composed h", **FWD)


_CHILD = r"""
import sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import node_embed_cases as NC
from egt_amd import _lib as L
from egt_amd.node_embed import node_embed_disabled
assert node_embed_disabled()
gpu = torch.device("cuda:0")
out = {{}}
for which in NC.MODEL_RUNS:
    r = NC.model_run(which, gpu, L.load())
    assert "k_node_embed" not in r["kernels"], r["kernels"]
    out[which] = dict(loss=r["loss"], grads=r["grads"])
torch.save(out, {out!r})
print("CHILD-OK")
"""


def test_switch_keeps_the_composed_ops_and_the_steps_agree(gpu, egt_lib, tmp_path):
    """EGT_NO_NODE_EMBED=1 is read once per process: a child process runs the five models on the composed ops; the losses
    (graph_loss, classification_loss) and every parameter gradient agree with the fused step"""
    src, out = tmp_path / "child.py", tmp_path / "composed.pt"
    src.write_text(_CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), out=str(out)))
    r = subprocess.run([sys.executable, str(src)], env=dict(os.environ, EGT_NO_NODE_EMBED="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, r.stdout + r.stderr
    composed = torch.load(out)
    for which in NC.MODEL_RUNS:
        fused = NC.model_run(which, gpu)
        assert_close(fused["loss"].reshape(1), composed[which]["loss"].double().reshape(1), name=f"{which}: loss", **FWD)
        assert set(fused["grads"]) == set(composed[which]["grads"])
        for k, g in composed[which]["grads"].items():
            assert_close(fused["grads"][k], g.double(), name=f"{which}: d {k}", **BWD)


def _zinc_run(tag, graph, tmp_path, gpu, random_neg, epochs=2):
    import egt_amd.training as T
    torch.manual_seed(0)
    cfg = dict(scheme="zinc.svd", model_width=64, edge_width=64, batch_size=8, model_name=tag, num_epochs=epochs, initial_lr=2e-3,
               use_svd=True, num_svd_features=16, sel_svd_features=8, random_neg=random_neg, num_virtual_nodes=1, model_height=2,
               upto_hop=4, random_mask_prob=0.0, use_hipgraph=graph, save_path=str(tmp_path / tag))
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
    mk = lambda n, seed: T.WithPositional(T.SyntheticZinc(n, 8, seed=seed, pad_multiple=1), "svd", 16)
    s.execute_training(mk(16, 1), mk(8, 2))
    return s


def test_use_hipgraph_reproduces_the_eager_zinc_svd_steps(tmp_path, gpu, egt_lib):
    """without the sign flip the step is a deterministic function of the weights and the batch: the replayed graph (the node
    embedding kernels inside it) reproduces the eager run bit for bit; with the flip (its draw is part of the graph) the graphed
    run trains"""
    eager, graphed = _zinc_run("e", False, tmp_path, gpu, False), _zinc_run("g", True, tmp_path, gpu, False)
    assert len(graphed._graphs) >= 1
    assert [h["loss"] for h in graphed.history] == [h["loss"] for h in eager.history] and len(eager.history) == 2
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
    flipped = _zinc_run("f", True, tmp_path, gpu, True, epochs=1)
    assert all(torch.isfinite(torch.tensor(h["loss"])) for h in flipped.history)


# ------------------------------------------------------------- the reference pin of the positional-encoding path -----
@pytest.mark.parametrize("name", ["zinc_svd", "zinc_eig"])
def test_model_matches_the_reference_with_positional_encodings(name, gpu, egt_lib):
    """the product model (its node input through the fused kernels), in inference mode as the fixture was written, against
    what the reference's own DCSVDTransformer(use_svd=True) / DCEigTransformer(use_eig=True) computed"""
    import cases as CS
    import node_embed_reference as NRF
    import virtual_nodes_ref as VR
    from egt_amd import ZincDCTransformer, mae_loss
    fix = NRF.load(name)
    c = NRF.CASES[name]
    cfg = dict(CS.MODEL_CASES[c["base"]]["cfg"], **c["pe"])
    model = ZincDCTransformer(random_mask_prob=0.0, random_neg=True, **cfg).to(gpu).eval()
    with torch.no_grad():
        for k, v in fix["weights"].items():
            prm = VR.module_param(model, k)
            if prm is not None:
                prm.copy_(v.to(gpu))
    inp = {k: v.to(gpu) for k, v in fix["inputs"].items()}
    pe = {k: inp[k] for k in ("singular_vectors", "eigen_vectors") if k in inp}
    h, _ = model.node_input(inp["node_features"].int(), **pe)
    assert type(h.grad_fn).__name__ == "_FusedNodeEmbedBackward"
    y = model(inp["node_features"].int(), inp["feature_matrix"].int(), inp["graph_matrix"], **pe)
    loss = mae_loss(y, inp["target"])
    loss.backward()
    assert_close(y, fix["out"]["y"], name=f"{name}: y", **FWD)
    assert_close(loss.reshape(1), fix["out"]["loss"], name=f"{name}: loss", **FWD)
    live = {id(p): k for k, p in model.keras_named_parameters().items()}
    checked = 0
    for k, r in fix["out"].items():
        if not k.startswith("d/"):
            continue
        prm = VR.module_param(model, k[2:])
        if prm is None or id(prm) not in live:
            assert float(r.abs().max()) == 0.0, f"{k}: the reference trains it, the model does not own it"
            continue
        assert_close(prm.grad, r, name=f"{name}: {k}", **BWD); checked += 1
    assert checked == len(live)
