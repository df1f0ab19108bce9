"""The CLUSTER / MNIST / ZINC-full schemes on the GPU: the CLUSTER model's classification_loss takes the fused node head and
agrees with the composed head (EGT_NO_NODE_HEAD=1 in a child process); the schemes train from the reference's config files
(tests/golden/schemes/) on synthetic graphs, resume, report, and replay from a hipGraph to the eager bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import assert_close, FWD, BWD

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "schemes")


def _fixture(rel, **over):
    return dict(json.load(open(os.path.join(GOLD, rel))), **over)


# ----------------------------------------------------------------------------- the fused route ---
def _cluster_step(device):
    """one classification_loss + backward of a 2-layer width-64 CLUSTER model on a fixed batch -> (arrays, route)"""
    from egt_amd import ClusterDCTransformer, class_weights_from_sizes, training as T
    torch.manual_seed(11)
    model = ClusterDCTransformer(model_width=64, edge_width=8, model_height=2, upto_hop=4, random_mask_prob=0.0).to(device)
    b = next(iter(T.SyntheticCluster(6, 6, nodes=(20, 44), seed=4)))
    w = class_weights_from_sizes(T.CLUSTER_CLASS_SIZES, device=device)
    loss, stats, aux = model.classification_loss(b["node_features"].to(device), b["graph_matrix"].to(device), b["target"].to(device), w)
    route = type(stats.grad_fn).__name__
    loss.backward()
    out = dict(loss=loss.detach().cpu().numpy(), stats=stats.detach().cpu().numpy())
    for k, p in model.keras_named_parameters().items():
        out["g:" + k] = p.grad.cpu().numpy()
    return out, route, aux


def _dump(path):
    out, route, _ = _cluster_step(torch.device("cuda:0"))
    np.savez(path, route=np.array(route), **out)


def test_cluster_model_takes_the_fused_route_and_agrees_with_the_composed_one(tmp_path, gpu, egt_lib):
    from egt_amd.node_head import node_head_disabled
    assert not node_head_disabled()
    got, route, aux = _cluster_step(gpu)
    assert route == "_FusedNodeHeadBackward" and aux == {}
    path = str(tmp_path / "composed.npz")
    env = dict(os.environ, EGT_NO_NODE_HEAD="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", f"import test_schemes_gpu as M; M._dump({path!r})"], env=env, cwd=HERE,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = np.load(path)
    assert str(ref["route"]) != route, "the switch keeps the composed head"
    assert_close(got["loss"], ref["loss"], name="loss", **FWD)
    assert_close(got["stats"][0], ref["stats"][0], name="stats[0]", **FWD)
    assert got["stats"][1:].tolist() == ref["stats"][1:].tolist()
    keys = [k for k in got if k.startswith("g:")]
    assert len(keys) >= 40 and "g:target/kernel" in keys and "g:node_norm_final/gamma" in keys
    for k in keys:
        assert_close(got[k], ref[k], name=k, **BWD)


# ------------------------------------------------------------------------------------- schemes ---
def _sets(T, s, which, n_train, n_val, bs):
    mk = {"cluster": lambda n, seed: T.SyntheticCluster(n, bs, nodes=(20, 44), seed=seed),
          "mnist": lambda n, seed: T.SyntheticMnist(n, bs, nodes=(20, 44), seed=seed),
          "zinc_full": lambda n, seed: T.SyntheticZinc(n, bs, seed=seed)}[which]
    c = s.config
    if c.get("use_eig"):
        return tuple(T.WithPositional(mk(n, sd), "eig", c.num_eig_features) for n, sd in ((n_train, 1), (n_val, 2)))
    if c.get("use_svd"):
        return tuple(T.WithPositional(mk(n, sd), "svd", c.num_svd_features) for n, sd in ((n_train, 1), (n_val, 2)))
    return mk(n_train, 1), mk(n_val, 2)


def test_cluster_svd_trains_resumes_and_reports(tmp_path, gpu, egt_lib):
    from egt_amd import training as T, ClusterDCTransformer
    cfg = _fixture("cluster/100k/egt.json", num_epochs=2, initial_lr=2e-3, batch_size=16, distributed=False, save_path=str(tmp_path / "run"))
    torch.manual_seed(0)
    s = T.import_scheme(cfg["scheme"])(cfg, device=gpu, print_fn=lambda *a: None)
    s.execute_training(*_sets(T, s, "cluster", 8 * 16, 2 * 16, 16))
    assert type(s.model) is ClusterDCTransformer and s.model.node_head_fused(torch.zeros(16, 44, 64, device=gpu))
    assert s.state.current_epoch == 2 and len(s.history) == 2
    for h in s.history:
        for k in ("loss", "xent", "val_loss", "val_xent", "val_acc"):
            assert k in h and h[k] == h[k], (k, h)
        assert 0.0 <= h["val_acc"] <= 1.0
    assert s.history[-1]["xent"] < s.history[0]["xent"] and s.history[-1]["val_xent"] < s.history[0]["val_xent"], s.history
    s2 = T.ClusterSVDScheme(dict(cfg, num_epochs=3), device=gpu, print_fn=lambda *a: None)
    s2.load_data(*_sets(T, s2, "cluster", 2 * 16, 16, 16)); s2.load_model(); s2.load_state()
    assert s2.state.current_epoch == 2 and s2.state.save_best_value == s.state.save_best_value
    assert torch.equal(s2.model.target.kernel, s.model.target.kernel)
    s2.train_model()
    assert s2.state.current_epoch == 3
    # the report, from the command line's --evaluate
    cfile = tmp_path / "cfg.json"
    cfile.write_text(json.dumps(cfg))
    T.main([str(cfile), "--synthetic", "32", "--evaluate"])
    for split in ("trainset", "valset", "testset"):
        lines = open(tmp_path / "run" / "predictions" / f"{split}_evals.txt").read().splitlines()
        assert [ln.split(" = ")[0] for ln in lines] == ["Accuracy", "Micro Recall", "Macro Recall", "Weighted Accuracy"], lines
        assert all(ln.endswith("%") and 0.0 <= float(ln.split(" = ")[1][:-1]) <= 100.0 for ln in lines)


@pytest.mark.parametrize("which,rel,keys,report", [
    ("cluster", "cluster/100k/egt_epe.json", ("loss", "val_loss", "val_acc"), "Accuracy = "),
    ("mnist", "mnist/100k/egt.json", ("loss", "xent", "val_xent", "val_acc"), "valset accuracy = "),
    ("zinc_full", "zinc_full/500k/egt_spe_do.json", ("loss", "mae", "distance_loss", "val_mae", "val_distance_loss"), "valset MAE = ")])
def test_scheme_trains_one_epoch_and_reports(which, rel, keys, report, tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    cfg = _fixture(rel, num_epochs=1, batch_size=16, distributed=False, save_path=str(tmp_path / "run"))
    torch.manual_seed(0)
    s = T.import_scheme(cfg["scheme"])(cfg, device=gpu, print_fn=lambda *a: None)
    tr, va = _sets(T, s, which, 4 * 16, 16, 16)
    s.execute_training(tr, va)
    assert s.state.current_epoch == 1 and len(s.history) == 1
    for k in keys:
        assert k in s.history[0] and np.isfinite(s.history[0][k]), (k, s.history)
    if which == "cluster":
        assert "xent" not in s.history[0] and "val_xent" not in s.history[0], "cluster.eig reports the accuracy only"
    if which == "zinc_full":
        assert s.model.dist_head is not None and s.config.distance_loss == 0.05 and s.history[0]["distance_loss"] > 0
    assert os.path.exists(tmp_path / "run" / "saved" / (cfg["model_name"] + ".npz"))
    s2 = T.import_scheme(cfg["scheme"])(dict(cfg, weight_file=""), device=gpu, print_fn=lambda *a: None)
    s2.do_evaluations(tr, va, None)
    lines = open(tmp_path / "run" / "predictions" / "valset_evals.txt").read().splitlines()
    assert lines and lines[0].startswith(report), lines


def test_use_hipgraph_reproduces_the_eager_cluster_run(tmp_path, gpu, egt_lib):
    """without the random mask the run is a deterministic function of the weights and the batches: the graphed run (fused node
    head inside the captured step) reproduces the eager run bit for bit"""
    from egt_amd import training as T

    def run(tag, graph):
        torch.manual_seed(0)
        cfg = _fixture("cluster/100k/egt.json", model_name=tag, num_epochs=2, initial_lr=2e-3, batch_size=8, distributed=False,
                       random_mask_prob=0.0, use_hipgraph=graph, save_path=str(tmp_path / tag))
        s = T.ClusterSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
        s.execute_training(*_sets(T, s, "cluster", 6 * 8, 8, 8))
        return s
    eager, graphed = run("e", False), run("g", True)
    assert len(graphed._graphs) >= 2
    assert [h["loss"] for h in graphed.history] == [h["loss"] for h in eager.history]
    assert [h["val_xent"] for h in graphed.history] == [h["val_xent"] for h in eager.history]
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
