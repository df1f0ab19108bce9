"""Graph-level readout head without a GPU: the exports and struct layouts, the library's coverage answers and refusals, the
composed head against the fp64 oracle (graph_head_ref.py) with the fairness conditions of every case the GPU tests use, the
models' graph_loss on CPU tensors (the composed path) against forward + loss + today's metric sums, and the schemes."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import graph_head_ref as GR
from util import assert_close, margin, FWD, BWD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(cid, "plain") for cid in GR.CASES] + [(cid, r) for cid in GR.RECIPE_CASES for r in GR.RECIPES]


def test_symbols_and_struct_layout(egt_lib, tmp_path):
    from egt_amd import _lib as L
    for name in ("egt_graph_head_supported", "egt_graph_head_workspace_bytes", "egt_graph_head_fwd", "egt_graph_head_bwd"):
        assert name in L._PROTOS and getattr(egt_lib, name) is not None
    assert L.ABI_VERSION == 4 and egt_lib.egt_abi_version() == 4
    pairs = [("egt_graph_head_desc", L.GraphHeadDesc), ("egt_node_head_params", L.NodeHeadParams)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("consts %d\\n", EGT_GH_LAYERNORM * 100 + EGT_GH_MAE * 10 + EGT_GH_XENT);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [f for f, _ in L.GraphHeadDesc._fields_] == ["B", "N", "W", "M0", "M1", "C", "nv", "loss", "activation", "flags", "ln_eps",
                                                       "reserved"]
    assert int(got["consts"]) == L.GH_LAYERNORM * 100 + L.GH_MAE * 10 + L.GH_XENT


def test_library_coverage(egt_lib):
    from egt_amd.graph_head import graph_head_desc, graph_head_supported
    for W in (48, 64):
        for m0, m1 in ((24, 12), (32, 16)):
            for Cn in (1, 2, 10, 16):
                for nv in (0, 1, 2, 4):
                    for act in ("elu", "relu"):
                        for loss in ("mae", "xent"):
                            for ln in (True, False):
                                d = graph_head_desc(3, 19, W, m0, m1, Cn, nv, loss, act, ln)
                                assert egt_lib.egt_graph_head_supported(C.byref(d)) == 1, (W, m0, m1, Cn, nv, act, loss, ln)
                                assert egt_lib.egt_graph_head_workspace_bytes(C.byref(d)) > 0
    assert graph_head_supported(128, 150, 64, 32, 16, 10, 0, "xent") and graph_head_supported(1, 1, 64, 32, 16, 1)
    for bad in (dict(W=80), dict(W=80, M0=40, M1=20), dict(M0=40, M1=20), dict(C_=17), dict(C_=0), dict(nv=17), dict(nv=-1),
                dict(activation="lrelu"), dict(N=0), dict(B=0)):
        kw = dict(B=3, N=19, W=64, M0=32, M1=16, C_=1, nv=0, loss="mae", activation="elu", layernorm=True)
        kw.update(bad)
        d = graph_head_desc(**kw)
        assert egt_lib.egt_graph_head_supported(C.byref(d)) == 0, bad
        assert egt_lib.egt_graph_head_workspace_bytes(C.byref(d)) == 0, bad
    d = graph_head_desc(3, 19, 64, 32, 16, 1); d.loss = 7
    assert egt_lib.egt_graph_head_supported(C.byref(d)) == 0 and egt_lib.egt_graph_head_workspace_bytes(C.byref(d)) == 0
    for nv in range(5, 17):                       # virtual-node counts the kernels do not flatten: answered, not guessed
        d = graph_head_desc(3, 19, 64, 32, 16, 1, nv)
        assert egt_lib.egt_graph_head_supported(C.byref(d)) == (egt_lib.egt_graph_head_workspace_bytes(C.byref(d)) > 0)
    d = graph_head_desc(1 << 16, (1 << 15) - 1, 64, 32, 16, 1, 1)             # B (nv + N) = 2^31
    assert egt_lib.egt_graph_head_supported(C.byref(d)) == 0
    d = graph_head_desc((1 << 16) - 1, (1 << 15) - 1, 64, 32, 16, 1, 1)       # just inside
    assert egt_lib.egt_graph_head_supported(C.byref(d)) == 1
    # the workspace: loss and hit of every graph, and one record per graph
    d = graph_head_desc(5, 19, 48, 24, 12, 3, 2, "xent")
    assert egt_lib.egt_graph_head_workspace_bytes(C.byref(d)) == 4 * 5 * (2 + 2 * 48 + 2 * 24 + 2 * 12 + 3 + 2 * 48)


def test_refusals_without_a_gpu(egt_lib):
    """argument checks run before any launch: error codes as the other entry points give them"""
    from egt_amd import _lib as L
    from egt_amd.graph_head import graph_head_desc, graph_head_loss
    ok = graph_head_desc(3, 19, 64, 32, 16, 1)
    noln_d = graph_head_desc(3, 19, 64, 32, 16, 1, layernorm=False)
    one = C.c_void_p(16)                                                       # any non-NULL value: never dereferenced here
    prm = L.NodeHeadParams(*([16] * 8))
    noln = L.NodeHeadParams(None, None, *([16] * 6))

    def fwd(d, p=prm, h=one, target=one, mask=one, stats=one, pred=one, ws=one):
        return egt_lib.egt_graph_head_fwd(C.byref(d) if d is not None else None, C.byref(p) if p is not None else None, h, target,
                                          mask, stats, pred, ws, None)

    def bwd(d, p=prm, g=prm, d_loss=one, d_h=one):
        return egt_lib.egt_graph_head_bwd(C.byref(d), C.byref(p), one, one, one, d_loss, d_h, C.byref(g) if g is not None else None,
                                          one, None)

    assert fwd(None) == L.EGT_E_NULL
    assert fwd(ok, p=None) == L.EGT_E_NULL
    for k in ("h", "target", "mask", "stats", "pred", "ws"):
        assert fwd(ok, **{k: None}) == L.EGT_E_NULL, k
    assert b"pred" in egt_lib.egt_last_error_string()
    assert fwd(ok, p=noln) == L.EGT_E_NULL and b"gamma/beta" in egt_lib.egt_last_error_string()
    assert bwd(ok, d_loss=None) == L.EGT_E_NULL and bwd(ok, d_h=None) == L.EGT_E_NULL and bwd(ok, g=None) == L.EGT_E_NULL
    assert bwd(ok, g=noln) == L.EGT_E_NULL
    assert bwd(noln_d, p=L.NodeHeadParams(None, None, 16, 16, None, 16, 16, 16), g=noln) == L.EGT_E_NULL   # NULL gamma / beta only
    d = graph_head_desc(3, 19, 64, 32, 16, 1); d.flags = 0x5
    assert fwd(d) == L.EGT_E_FLAGS and bwd(d) == L.EGT_E_FLAGS and egt_lib.egt_graph_head_supported(C.byref(d)) == 0
    d = graph_head_desc(3, 19, 64, 32, 16, 1); d.reserved = 1
    assert fwd(d) == L.EGT_E_FLAGS
    d = graph_head_desc(3, 19, 64, 32, 16, 1); d.loss = 7
    assert fwd(d) == L.EGT_E_FLAGS and b"EGT_GH_MAE" in egt_lib.egt_last_error_string()
    assert fwd(graph_head_desc(3, 19, 80, 32, 16, 1)) == L.EGT_E_SHAPE and b"{48,64}" in egt_lib.egt_last_error_string()
    assert fwd(graph_head_desc(3, 19, 64, 40, 20, 1)) == L.EGT_E_SHAPE and b"(M0, M1)" in egt_lib.egt_last_error_string()
    assert fwd(graph_head_desc(3, 19, 64, 32, 16, 17)) == L.EGT_E_SHAPE and bwd(graph_head_desc(3, 19, 64, 32, 16, 0)) == L.EGT_E_SHAPE
    assert fwd(graph_head_desc(3, 19, 64, 32, 16, 1, 17)) == L.EGT_E_SHAPE and b"virtual" in egt_lib.egt_last_error_string()
    assert fwd(graph_head_desc(0, 19, 64, 32, 16, 1)) == L.EGT_E_SHAPE
    with pytest.raises(AssertionError):
        L.check(L.EGT_E_SHAPE)
    # the Python operator: dtype and device errors before the library is asked to launch
    c = GR.make_case("w64_xent_n19")
    with pytest.raises(TypeError):
        graph_head_loss(c["h"], c["target"].float(), c["mask"], c["params"], "xent")
    with pytest.raises((ValueError, RuntimeError, TypeError)):
        graph_head_loss(c["h"], c["target"], c["mask"], c["params"], "xent")        # CPU tensors: no fallback inside the fused op


@pytest.mark.parametrize("cid,recipe", ALL, ids=[f"{a}-{b}" for a, b in ALL])
def test_composed_head_equals_the_oracle_and_the_case_is_fair(cid, recipe):
    """the composed fp32 head on the CPU stays within CAP of every tolerance the GPU tests apply to the case, and the oracle's
    predictions keep their distance from the kinks of the two losses"""
    from egt_amd.graph_head import graph_head_composed
    c, ref = GR.reference(cid, recipe)
    assert ref["fair"] >= 1e-3, f"{cid}/{recipe}: min |y - t| (MAE) / top-2 logit gap (XENT) is {ref['fair']:.2e}: draw another seed"
    got, st = GR.run(graph_head_composed, c)
    assert st.shape == (3,) and st.dtype == torch.float32 and got["pred"].shape == (c["B"], c["C"])
    assert got["stats"][1:].tolist() == ref["stats"][1:].tolist(), "counts are exact"
    assert float(got["stats"][2]) == (c["B"] * c["C"] if c["loss"] == "mae" else c["B"])
    worst = {"loss": margin(got["stats"][:1], ref["stats"][:1], rtol=FWD["rtol"], arel=FWD["arel"]),
             "pred": margin(got["pred"], ref["pred"], rtol=FWD["rtol"], arel=FWD["arel"]),
             "d_h": margin(got["d_h"], ref["d_h"], rtol=BWD["rtol"], arel=BWD["arel"])}
    for n, a, r in zip(GR.grad_names(c), got["grads"], ref["grads"]):
        worst[n] = margin(a, r, rtol=BWD["rtol"], arel=BWD["arel"])
    bad = {k: round(v, 3) for k, v in worst.items() if not v <= GR.CAP}
    assert not bad, f"{cid}/{recipe}: the composed fp32 head uses more than {GR.CAP} of the tolerance: {bad}"
    zero = GR.zero_rows(c)
    if bool(zero.any()):
        assert float(got["d_h"][zero].abs().max()) == 0.0
    # the composed head in fp64 IS the oracle
    p64 = tuple(None if p is None else p.double() for p in c["params"])
    st_d, y_d = graph_head_composed(c["h"].double(), c["target"], c["mask"], p64, c["loss"], c["nv"], c["act"])
    assert_close(st_d, ref["stats"], name="fp64 composed stats", rtol=1e-12, arel=1e-12)
    assert_close(y_d, ref["pred"], name="fp64 composed pred", rtol=1e-12, arel=1e-12)


def test_case_table_is_the_issues():
    """the shapes at which the kernels can go wrong: each property the table claims holds for the generated inputs"""
    c = GR.make_case("w64_mae_b70")
    n = c["mask"].sum(1)
    assert c["B"] == 70 and int(n.min()) >= 1 and int(n.max()) <= 6 and len(n.unique()) > 1
    for cid in GR.CASES:
        c = GR.make_case(cid)
        assert c["h"].shape == (c["B"], c["nv"] + c["N"], c["W"]) and c["mask"].shape == c["h"].shape[:2]
        assert bool(c["mask"][:, :c["nv"]].all()) and int(c["mask"].sum(1).min()) >= c["nv"] + 1
        assert c["params"][2].shape == (max(c["nv"], 1) * c["W"], c["M0"])
    assert GR.make_case("w64_mae_relu_noln")["params"][0] is None
    assert GR.make_case("w64_mae_1x1")["h"].shape == (1, 1, 64)
    for r in GR.RECIPES:
        assert not torch.equal(GR.make_case("w64_mae_n19", r)["h"], GR.make_case("w64_mae_n19")["h"])


class _Pass(torch.nn.Module):
    """stands in for the layers of a model on the CPU (the attention blocks have no CPU path)"""

    def forward(self, h, e, mask, attn_mask, skip_last_edge_ffn=True):
        return h, e


def _cpu_model(cls, h, mask, **kw):
    """a model whose embeddings / layers are replaced by fixed tensors: forward and graph_loss share them"""
    model = cls(model_width=h.shape[-1], edge_width=8, model_height=1, upto_hop=2, random_mask_prob=0.0, **kw)
    e = torch.zeros(h.shape[0], h.shape[1], h.shape[1], 8)
    model.embeddings = lambda nf, fm, adj: (h, e, mask)
    model.layers = _Pass()
    return model


@pytest.mark.parametrize("which,cid", [("zinc", "w64_mae_n19"), ("cifar10", "w64_xent_n19")])
def test_graph_loss_on_cpu_equals_forward_plus_loss(which, cid, egt_lib):
    from egt_amd import Cifar10DCTransformer, ZincDCTransformer, mae_loss, sparse_xent_loss
    c = GR.make_case(cid)
    torch.manual_seed(3)
    model = _cpu_model(Cifar10DCTransformer if which == "cifar10" else ZincDCTransformer, c["h"], c["mask"])
    assert model.target.kernel.shape[1] == c["C"] and model.GRAPH_LOSS == c["loss"]
    with torch.no_grad():
        for p in model.graph_head_params():
            p.add_(0.1 * torch.randn_like(p))
    assert not model.graph_head_fused(c["h"]), "CPU tensors take the composed head"
    nf = fm = adj = torch.zeros(1)
    tgt = c["target"]
    loss, stats, pred, aux = model.graph_loss(nf, fm, adj, tgt)
    assert aux == {} and stats.shape == (3,) and not pred.requires_grad
    g_new = torch.autograd.grad(loss, list(model.graph_head_params()))
    y = model(nf, fm, adj)                                                  # today's batch_loss: forward + loss_fn + the metric sums
    old = (sparse_xent_loss if which == "cifar10" else mae_loss)(y, tgt)
    g_old = torch.autograd.grad(old, list(model.graph_head_params()))
    tight = dict(rtol=1e-5, arel=1e-6)                                      # fp32 sums in another order
    assert_close(loss, old, name="loss", **tight)
    assert_close(pred, y, name="pred", **tight)
    st = stats.detach()
    if which == "cifar10":
        n = tgt.numel()
        assert_close(st[0], old.detach() * n, name="xent sum", **tight)
        assert float(st[1]) == float((y.argmax(-1) == tgt).sum()) and float(st[2]) == n
    else:
        assert_close(st[0], (y - tgt).abs().sum().detach(), name="sabs", **tight)
        assert float(st[1]) == 0.0 and float(st[2]) == tgt.numel()
    for a, b, n in zip(g_new, g_old, GR.NAMES):
        assert_close(a, b, name=n, **tight)


def test_per_node_models_do_not_get_the_method():
    from egt_amd import ClusterDCTransformer, MnistDCTransformer, PatternDCTransformer, ZincDCTransformer
    for cls in (PatternDCTransformer, ClusterDCTransformer):
        m = cls(model_width=16, edge_width=8, model_height=1, upto_hop=2)
        assert not hasattr(m, "graph_loss") and not hasattr(m, "graph_head_fused") and hasattr(m, "classification_loss")
    assert ZincDCTransformer.GRAPH_LOSS == "mae" and MnistDCTransformer.GRAPH_LOSS == "xent"
    assert hasattr(MnistDCTransformer(model_width=16, model_height=1, upto_hop=2), "graph_loss")


class _Stub(torch.nn.Module):
    """a model_factory stub: no graph_loss, so the schemes keep today's path"""

    def __init__(self, out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(out))

    def forward(self, nf, fm, adj, **kw):
        return adj.sum((1, 2))[:, None] * 0.01 + self.w[None, :]


@pytest.mark.parametrize("which", ["zinc", "cifar10"])
def test_scheme_with_a_stub_model_still_trains(which, tmp_path):
    import egt_amd.training as T
    if which == "zinc":
        cls, data, out = T.ZincSVDScheme, T.SyntheticZinc(16, 8, seed=1), 1
    else:
        cls, data, out = T.Cifar10SVDScheme, T.SyntheticCifar10(16, 8, nodes=(10, 14), seed=1), 10
    s = cls(dict(scheme=f"{which}.svd", model_name="stub", num_epochs=2, initial_lr=0.05, batch_size=8, use_svd=False,
                 save_path=str(tmp_path / "run")), model_factory=lambda mc: _Stub(out), print_fn=lambda *a: None)
    s.execute_training(data, data)
    assert not hasattr(s.model, "graph_loss")
    assert len(s.history) == 2 and s.history[-1]["loss"] < s.history[0]["loss"]
    b = next(iter(data))
    loss, ms = s.batch_loss(b)
    assert set(ms) == ({"mae", "loss"} if which == "zinc" else {"xent", "acc", "loss"})


@pytest.mark.parametrize("which,cid", [("zinc", "w64_mae_n19"), ("cifar10", "w64_xent_n19")])
def test_scheme_metric_sums_keep_their_meaning(which, cid, tmp_path, egt_lib):
    """batch_loss through graph_loss: the same names and (sum, count) pairs as the arithmetic on forward's output"""
    import egt_amd.training as T
    from egt_amd import Cifar10DCTransformer, ZincDCTransformer
    c = GR.make_case(cid)
    torch.manual_seed(4)
    model = _cpu_model(Cifar10DCTransformer if which == "cifar10" else ZincDCTransformer, c["h"], c["mask"])
    cls = T.Cifar10SVDScheme if which == "cifar10" else T.ZincSVDScheme
    s = cls(dict(scheme=f"{which}.svd", model_name="m", batch_size=3, use_svd=False, save_path=str(tmp_path / "run")),
            print_fn=lambda *a: None)
    s.model, s.loss_fn = model, s.get_loss()
    z = torch.zeros(1)
    batch = dict(node_features=z, feature_matrix=z, graph_matrix=z, target=c["target"])
    loss, ms = s.batch_loss(batch)
    y = model(z, z, z)
    tight = dict(rtol=1e-5, arel=1e-6)
    assert_close(loss, s.loss_fn(y, c["target"]), name="loss", **tight)
    val = {k: float(a) / float(b) for k, (a, b) in ms.items()}
    if which == "zinc":
        want = float((y - c["target"]).abs().mean().detach())
        assert set(ms) == {"mae", "loss"} and float(ms["mae"][1]) == c["target"].numel()
        assert abs(val["mae"] - want) <= 1e-5 * want and abs(val["loss"] - want) <= 1e-5 * want
    else:
        n = c["target"].numel()
        assert set(ms) == {"xent", "acc", "loss"} and float(ms["acc"][1]) == n and float(ms["xent"][1]) == n
        assert val["acc"] == float((y.argmax(-1) == c["target"]).sum()) / n
        lv = float(loss.detach())
        assert abs(val["xent"] - lv) <= 1e-5 * lv and abs(val["loss"] - lv) <= 1e-5 * lv
