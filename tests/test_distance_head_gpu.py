"""Distance objective on the GPU: the target kernel (bit-exact), the fused edge-head loss kernels against fp64 autograd of the
restatement in distance_ref.py, the C-ABI refusals, the models with the objective on, and the zinc.svd / cifar10.svd schemes
from the reference's egt_spe_do configs (tests/golden/distance/)."""
import ctypes as C
import json
import os

import pytest
import torch

import distance_ref as DR
from util import assert_close, bf16_stack_tol, FWD, BWD

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distance")

N0 = 19                                    # 361 pairs per graph: 22 full tiles and a ragged one; two workgroups per graph
ADJ = DR.make_graphs(N0)                   # shared, never modified
TARGETS = {T: DR.ref_target(ADJ, T) for T in (1, 3, 8)}


def test_inputs_exercise_the_tiling():
    for T, t in TARGETS.items():
        assert sorted(t.unique().tolist()) == list(range(T + 1)), "every class 0..T occurs"
        zero, mixed = DR.tile_census(t[0])
        assert zero >= 1 and mixed >= 1
    assert DR.tile_census(TARGETS[3][0]) == (4, 19)
    assert int(TARGETS[8][2].abs().max()) == 0


@pytest.mark.parametrize("T", [1, 3, 8])
def test_target_is_bit_exact(T, gpu, egt_lib):
    from egt_amd import distance_target
    got = distance_target(ADJ.to(gpu), T)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu().long(), TARGETS[T])
    assert torch.equal(distance_target(ADJ, T).long(), TARGETS[T]), "the CPU form of distance_target"


def test_target_larger_graphs(gpu, egt_lib):
    """more than one row tile per wave and several column blocks: N = 70 and N = 150 (the CIFAR10 size), random graphs"""
    from egt_amd import distance_target
    for B, N, T in ((2, 70, 5), (3, 150, 3)):
        g = torch.Generator().manual_seed(N)
        adj = (torch.rand(B, N, N, generator=g) > 0.97).float()
        adj = ((adj + adj.transpose(1, 2)) > 0).float()
        assert torch.equal(distance_target(adj.to(gpu), T).cpu().long(), DR.ref_target(adj, T))


def _run_case(gpu, De, width, T, act, layernorm=True, dtype=torch.float32, N=N0, seed=0):
    from egt_amd.head import distance_head, distance_head_composed
    adj = ADJ if N == N0 else DR.make_graphs(N)
    target = TARGETS[T] if N == N0 else DR.ref_target(adj, T)
    B = adj.shape[0]
    g = torch.Generator().manual_seed(7 + seed)
    e = torch.randn(B, N, N, De, generator=g) * 1.5 + 0.3
    if dtype == torch.bfloat16:
        e = e.to(torch.bfloat16).float()                     # the reference sees the same bf16-rounded e
    s = torch.tensor([0.7, -1.3, 0.45][:B])                  # a non-uniform upstream gradient of per_graph
    params = DR.head_params(De, width, T, layernorm, seed)
    # fp64 autograd of the restatement
    e64 = e.double().requires_grad_()
    p64 = tuple(None if p is None else p.double().requires_grad_() for p in params)
    pg64 = DR.ref_head(e64, target, p64, act)
    live = [p for p in p64 if p is not None]
    gr = torch.autograd.grad(pg64, [e64] + live, s.double())
    # fused
    eg = e.to(gpu).to(dtype).requires_grad_()
    pg_ = tuple(None if p is None else p.to(gpu).requires_grad_() for p in params)
    tg = target.to(torch.uint8).to(gpu)
    out = distance_head(eg, tg, pg_, act)
    out.backward(s.to(gpu))
    got = dict(per_graph=out.detach(), d_e=eg.grad, grads=[p.grad for p in pg_ if p is not None])
    ref = dict(per_graph=pg64.detach(), d_e=gr[0], grads=list(gr[1:]), target=target)
    # composed torch ops on the GPU: the A/B baseline computes the same thing
    ec = e.to(gpu).requires_grad_()
    pc = tuple(None if p is None else p.to(gpu).requires_grad_() for p in params)
    oc = distance_head_composed(ec, tg, pc, act)
    oc.backward(s.to(gpu))
    comp = dict(per_graph=oc.detach(), d_e=ec.grad, grads=[p.grad for p in pc if p is not None])
    return got, ref, comp, (eg, tg, pg_, s)


def _check(got, ref, comp, dtype=torch.float32, names=DR.HEAD_NAMES):
    de_tol = bf16_stack_tol(1) if dtype == torch.bfloat16 else BWD
    for other, tag in ((ref, "fp64"), (comp, "composed")):
        assert_close(got["per_graph"], other["per_graph"], name=f"per_graph vs {tag}", **FWD)
        assert_close(got["d_e"].float(), other["d_e"], name=f"d_e vs {tag}", **de_tol)
        for n, a, r in zip(names, got["grads"], other["grads"]):
            assert_close(a, r, name=f"d {n} vs {tag}", **BWD)
    t = ref["target"].to(got["d_e"].device)
    assert float(got["per_graph"][2]) == 0.0 and float(got["d_e"][2].abs().max()) == 0.0, "the graph without edges"
    assert float(got["d_e"][t == 0].abs().max()) == 0.0, "no gradient where the target is 0"
    assert float(got["d_e"][t > 0].abs().max()) > 0.0


CASES = [(48, 48, 3, "elu", True), (64, 64, 8, "elu", True), (8, 64, 3, "relu", True), (16, 64, 3, "elu", False),
         (32, 64, 3, "elu", True)]           # De = 32: the two-tile instance of the shared tile body


@pytest.mark.parametrize("De,width,T,act,ln", CASES)
def test_head_forward_backward(De, width, T, act, ln, gpu, egt_lib):
    got, ref, comp, _ = _run_case(gpu, De, width, T, act, ln)
    names = DR.HEAD_NAMES if ln else DR.HEAD_NAMES[2:]
    _check(got, ref, comp, names=names)


def test_head_bf16_edges(gpu, egt_lib):
    got, ref, comp, _ = _run_case(gpu, 8, 64, 3, "relu", True, dtype=torch.bfloat16)
    assert got["d_e"].dtype == torch.bfloat16
    _check(got, ref, comp, dtype=torch.bfloat16)


def test_head_full_tiles(gpu, egt_lib):
    """N = 16: every tile is full (256 pairs per graph = 16 tiles)"""
    got, ref, comp, _ = _run_case(gpu, 64, 64, 3, "elu", True, N=16)
    _check(got, ref, comp)


def test_two_calls_are_bitwise_equal(gpu, egt_lib):
    from egt_amd.head import distance_head
    _, _, _, (eg, tg, params, s) = _run_case(gpu, 64, 64, 8, "elu", True)
    runs = []
    for _ in range(2):
        e = eg.detach().clone().requires_grad_()
        ps = tuple(p.detach().clone().requires_grad_() for p in params)
        out = distance_head(e, tg, ps, "elu")
        out.backward(s.to(gpu))
        runs.append([out.detach(), e.grad] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_capi_refusals(gpu, egt_lib):
    from egt_amd import _lib as L
    from egt_amd.head import head_desc
    ok = head_desc(2, 19, 64, 32, 16, 4)
    assert egt_lib.egt_edge_head_supported(C.byref(ok)) == 1 and egt_lib.egt_edge_head_workspace_bytes(C.byref(ok)) > 0
    buf = torch.zeros(1 << 16, device=gpu)
    prm = L.HeadParams(*([buf.data_ptr()] * 8))
    st = L.current_stream()

    def fwd(d, target=buf):
        return egt_lib.egt_edge_head_fwd(C.byref(d), C.byref(prm), L.ptr(buf), L.ptr(target), L.ptr(buf), L.ptr(buf), st)

    d = head_desc(2, 19, 64, 32, 16, 4); d.flags = 0x5
    assert fwd(d) == L.EGT_E_FLAGS and egt_lib.egt_edge_head_supported(C.byref(d)) == 0
    d = head_desc(2, 19, 64, 32, 16, 4); d.reserved = 1
    assert fwd(d) == L.EGT_E_FLAGS
    assert fwd(ok, target=None) == L.EGT_E_NULL
    assert b"target" in egt_lib.egt_last_error_string()
    assert egt_lib.egt_edge_head_bwd(C.byref(ok), C.byref(prm), L.ptr(buf), None, L.ptr(buf), L.ptr(buf), C.byref(prm), L.ptr(buf),
                                     st) == L.EGT_E_NULL
    d = head_desc(2, 19, 64, 32, 16, 17)
    assert fwd(d) == L.EGT_E_SHAPE and egt_lib.egt_edge_head_workspace_bytes(C.byref(d)) == 0
    d = head_desc(2, 19, 64, 8, 16, 4)
    assert fwd(d) == L.EGT_E_SHAPE and b"(M0, M1)" in egt_lib.egt_last_error_string()
    assert egt_lib.egt_distance_target(None, 2, 19, 3, L.ptr(buf), st) == L.EGT_E_NULL
    assert egt_lib.egt_distance_target(L.ptr(buf), 2, 19, 0, L.ptr(buf), st) == L.EGT_E_SHAPE


# ------------------------------------------------------------------------------------ models -----
def _head_oracle_names():
    return [n.replace("/", ".") for n in DR.HEAD_NAMES[2:]]


def _add_head_params(params, De, width, T, seed=0):
    """the oracle parameter dict (MO.init_zinc_params) + the head's Dense layers; edge_norm_final.* is already in it"""
    hp = DR.head_params(De, width, T, True, seed)
    for n, v in zip(_head_oracle_names(), hp[2:]):
        params[n] = v
    return params


def _load_head(model, params):
    with torch.no_grad():
        head = model.dist_head
        head.edge_norm_final.gamma.copy_(params["edge_norm_final.gamma"]); head.edge_norm_final.beta.copy_(params["edge_norm_final.beta"])
        named = head.keras_named_parameters()
        for n in DR.HEAD_NAMES[2:]:
            named[n].copy_(params[n.replace("/", ".")])


def _head_terms(e_f, adj, p64, T, act="elu"):
    return DR.ref_mlp_loss(e_f, DR.ref_target(adj, T), *[p64[n] for n in _head_oracle_names()], act)


def _check_model_grads(model, gro, ptol, checked_min):
    """every parameter gradient against fp64 autograd; the formerly dead ones and the head's must be there and non-zero"""
    from test_model import _grad_of
    Ly = len(model.layers.blocks)
    named = model.keras_named_parameters()
    live = [f"layer{Ly - 1}.dense_edge_r.kernel", f"layer{Ly - 1}.dense_edge_r.bias", f"layer{Ly - 1}.ffn_edge.lr1_kernel",
            f"layer{Ly - 1}.ffn_edge.lr2_bias", f"layer{Ly - 1}.ffn_edge.norm_gamma", "edge_norm_final.gamma", "edge_norm_final.beta"] \
        + _head_oracle_names()
    checked = 0
    for k, gref in gro.items():
        if k.startswith("edge_norm_final.") or k.startswith("mlp_out_dist_targ_") or k.startswith("distance_target."):
            prm = named[k.replace(".", "/")]
        elif k.startswith("node_emb.") or k.startswith("edge_emb."):
            prm = getattr(getattr(model, k.split(".")[0]), k.split(".")[1], None) if not isinstance(model.node_emb, torch.nn.Parameter) \
                or k.startswith("edge_emb.") else model.node_emb
        else:
            prm = _grad_of(model, k)
        if prm is None or gref is None:
            assert k not in live, k
            continue
        if k in live:
            assert float(gref.abs().max()) > 1e-6 and float(prm.grad.abs().max()) > 0.0, f"{k}: live with the objective on"
        assert_close(prm.grad, gref, name=k, **ptol)
        checked += 1
    assert checked >= checked_min, checked


def test_zinc_model_with_the_distance_objective(gpu, egt_lib, tmp_path):
    from egt_amd import ZincDCTransformer, mae_loss
    from oracle import egt_model_oracle as MO
    from test_model import _load_params
    cfg = dict(model_width=48, edge_width=48, model_height=2, upto_hop=4)
    w, T, B, N = 0.05, 3, 2, 12
    g = torch.Generator().manual_seed(12)
    n = torch.tensor([12, 9]); real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
    adj = (torch.rand(B, N, N, generator=g) > 0.75).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
    y = torch.randn(B, 1, generator=g)
    params = _add_head_params(MO.init_zinc_params(cfg, dtype=torch.float32, generator=g), 48, 48, T)
    model = ZincDCTransformer(random_mask_prob=0.0, distance_loss=w, distance_target=T, **cfg).to(gpu).eval()
    _load_params(model, params, gpu); _load_head(model, params)
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    yo, _, e_f, _ = MO.zinc_forward(nf, fm, adj, p64, cfg, return_hidden=True)
    pgo = _head_terms(e_f, adj, p64, T)
    loss_o = MO.mae_loss(yo, y.double()) + w * pgo.mean()
    gro = dict(zip(p64, torch.autograd.grad(loss_o, list(p64.values()), allow_unused=True)))
    pred, aux = model(nf.to(gpu), fm.to(gpu), adj.to(gpu), return_aux=True)
    assert torch.equal(pred, model(nf.to(gpu), fm.to(gpu), adj.to(gpu))), "the default return value is the prediction"
    (mae_loss(pred, y.to(gpu)) + w * aux["distance_loss"].mean()).backward()
    assert_close(pred, yo, name="prediction", rtol=2e-4, arel=5e-5)
    assert_close(aux["distance_loss"], pgo, name="distance_loss per graph", rtol=2e-4, arel=5e-5)
    _check_model_grads(model, gro, BWD, 60)
    # names and the npz round trip
    named = model.keras_named_parameters()
    for k in DR.HEAD_NAMES + ("dense_edge_r_01/kernel", "fnn_lr1_edge_01/kernel", "norm_fnn_edge_01/beta"):
        assert k in named, k
    from egt_amd import training as TR
    s = TR.ZincSVDScheme(dict(scheme="zinc.svd", use_svd=False, distance_loss=w, distance_target=T, save_path=str(tmp_path), **cfg),
                         device=gpu, print_fn=lambda *a: None)
    s.load_model()
    with torch.no_grad():
        for k, v in s.model.keras_named_parameters().items():
            v.copy_(named[k])
    s.save_weights(str(tmp_path / "w.npz"))
    with torch.no_grad():
        for v in s.model.keras_named_parameters().values():
            v.zero_()
    s.load_weights(str(tmp_path / "w.npz"))
    for k, v in s.model.keras_named_parameters().items():
        assert torch.equal(v, named[k]), k


@pytest.mark.parametrize("edge_dtype", ["f32", "bf16"])
def test_cifar10_model_with_the_distance_objective(edge_dtype, gpu, egt_lib):
    from egt_amd import Cifar10DCTransformer, sparse_xent_loss
    from oracle import egt_model_oracle as MO, egt_oracle as O
    from test_model import _load_params
    bf = edge_dtype == "bf16"
    if bf:
        from test_block_gpu import _Bf16Storage
    S = _Bf16Storage.apply if bf else (lambda t: t)           # the oracle rounds e where the model stores it
    Ly, w, T, B, N = 2, 0.0005, 3, 2, 18
    cfg = dict(model_width=64, edge_width=8, model_height=Ly, upto_hop=4, num_node_features=1, num_edge_features=0, num_targets=10,
               float_node_features=5, float_edge_features=1)
    g = torch.Generator().manual_seed(18)
    n = torch.tensor([18, 11]); real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
    adj = (torch.rand(B, N, N, generator=g) > 0.7).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
    y = torch.randint(0, 10, (B,), generator=g)
    params = _add_head_params(MO.init_zinc_params(cfg, dtype=torch.float32, generator=g), 8, 64, T)
    model = Cifar10DCTransformer(model_width=64, model_height=Ly, upto_hop=4, random_mask_prob=0.0, distance_loss=w,
                                 distance_target=T, edge_dtype=edge_dtype).to(gpu).eval()
    _load_params(model, params, gpu); _load_head(model, params)
    p64 = {k: v.double().requires_grad_() for k, v in params.items() if k not in ("fm_emb.embeddings", "node_emb.embeddings")}
    xn, mask = MO.keras_masking(nf.double(), -1.0)                                          # cifar10_forward, layer by layer
    h = O.dense(xn, p64["node_emb.kernel"], p64["node_emb.bias"])
    xe, _ = MO.keras_masking(fm.double(), -1.0)
    e = O.dense(xe, p64["edge_emb.kernel"], p64["edge_emb.bias"])
    e = S(e + O.dense(MO.stack_hops(adj.double(), cfg["upto_hop"]), p64["adj_emb.kernel"], p64["adj_emb.bias"]))
    for ii in range(Ly):
        bp = {k[len(f"layer{ii}."):]: v for k, v in p64.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
        h, e = O.block_forward(h, e, mask, bp, num_heads=8)
        fn = {k.split(".", 2)[2]: v for k, v in p64.items() if k.startswith(f"layer{ii}.ffn_node.")}
        fe = {k.split(".", 2)[2]: v for k, v in p64.items() if k.startswith(f"layer{ii}.ffn_edge.")}
        e = S(O.ffn_forward(S(e), fe))                                                      # the last layer's edge FFN is live
        h = O.ffn_forward(h, fn)
    h = O.layer_norm(h, p64["node_norm_final.gamma"], p64["node_norm_final.beta"])
    e_f = O.layer_norm(e, p64["edge_norm_final.gamma"], p64["edge_norm_final.beta"])
    lo = O.dense(MO.mlp_out(MO.masked_global_avg_pool_1d(h, mask), p64, 2, "elu"), p64["target.kernel"], p64["target.bias"])
    pgo = _head_terms(e_f, adj, p64, T)
    loss_o = MO.sparse_xent_loss(lo, y) + w * pgo.mean()
    gro = dict(zip(p64, torch.autograd.grad(loss_o, list(p64.values()), allow_unused=True)))
    logits, aux = model(nf.to(gpu), fm.to(gpu), adj.to(gpu), return_aux=True)
    (sparse_xent_loss(logits, y.to(gpu)) + w * aux["distance_loss"].mean()).backward()
    tol = bf16_stack_tol(1) if bf else dict(rtol=2e-4, arel=5e-5)
    assert_close(logits, lo, name="logits", **tol)
    assert_close(aux["distance_loss"], pgo, name="distance_loss per graph", **tol)
    _check_model_grads(model, gro, bf16_stack_tol(1, params=True) if bf else BWD, 60)


# ------------------------------------------------------------------------------------ schemes -----
def _fixture(name, **over):
    return dict(json.load(open(os.path.join(GOLD, name + ".json"))), **over)


def _sets(T, s, which, n_train, n_val, bs):
    if which == "zinc":
        mk = lambda n, seed: T.SyntheticZinc(n, bs, seed=seed, pad_multiple=1)
    else:
        mk = lambda n, seed: T.SyntheticCifar10(n, bs, nodes=(20, 44), seed=seed, pad_multiple=1)
    if s.config.get("use_svd"):
        base, nsvd = mk, s.config.num_svd_features
        mk = lambda n, seed: T.WithPositional(base(n, seed), "svd", nsvd)
    return mk(n_train, 1), mk(n_val, 2)


@pytest.mark.parametrize("which,name,base,w", [("zinc", "zinc_100k_egt_spe_do", "mae", 0.05),
                                               ("cifar10", "cifar10_100k_egt_spe_do", "xent", 0.0005)])
def test_scheme_trains_the_reference_spe_do_config(which, name, base, w, tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    cls = T.ZincSVDScheme if which == "zinc" else T.Cifar10SVDScheme

    def run(tag, **over):
        torch.manual_seed(0)
        cfg = _fixture(name, model_name=tag, num_epochs=2, steps_per_epoch=6, distributed=False, save_path=str(tmp_path / tag), **over)
        s = cls(cfg, device=gpu, print_fn=lambda *a: None)
        assert s.config.distance_loss == w and s.config.distance_target == 3
        s.execute_training(*_sets(T, s, which, 6 * 16, 2 * 16, 16))
        return s

    s = run("fixture")
    assert s.model.dist_head is not None and len(s.history) == 2
    for h in s.history:
        for k in ("loss", base, "distance_loss", "val_loss", "val_" + base, "val_distance_loss"):
            assert k in h and h[k] == h[k], (k, h)
        assert abs(h["val_loss"] - (h["val_" + base] + w * h["val_distance_loss"])) <= 1e-5 * abs(h["val_loss"]), h
        assert abs(h["loss"] - (h[base] + w * h["distance_loss"])) <= 1e-4 * abs(h["loss"]), h
        assert h["distance_loss"] > 0 and h["val_distance_loss"] > 0
    assert s.history[-1]["loss"] < s.history[0]["loss"], "the training loss falls"
    # config.use_hipgraph: without the random mask and the random sign flip the run is a deterministic function of the weights
    # and the batches, so the graphed run reproduces the eager run's history exactly (tests/test_training.py's criterion)
    det = dict(random_mask_prob=0.0, random_neg=False)
    eager, graphed = run("e", use_hipgraph=False, **det), run("g", use_hipgraph=True, **det)
    assert len(graphed._graphs) >= 1
    assert [h["loss"] for h in graphed.history] == [h["loss"] for h in eager.history]
    assert [h["distance_loss"] for h in graphed.history] == [h["distance_loss"] for h in eager.history]
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
