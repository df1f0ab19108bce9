"""Virtual nodes on the GPU: the bordered edge embedding (egt_edge_embed_vn_fwd/bwd) against the plain embedding bit for
bit and against the fp64 restatement (virtual_nodes_ref.py), the ZINC / CIFAR10 models with num_virtual_nodes > 0 against the
restatement (prediction and every named parameter's gradient), padding invariance, and the training driver (checkpoint
resume, one hipGraph step)."""
import math

import numpy as np
import pytest
import torch

import virtual_nodes_ref as VR
from util import assert_close, bf16_stack_tol, FWD, BWD

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _embed_inputs(B, N, De, K, nv, F, seed):
    g = torch.Generator().manual_seed(seed)
    adj = (torch.rand(B, N, N, generator=g) > 0.8).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float()
    V = 1 if F else 5
    fm = torch.full((B, N, N), -1) if F else torch.where(adj > 0, torch.randint(0, V - 1, (B, N, N), generator=g), torch.tensor(-1))
    p = dict(table=torch.zeros(1, De) if F else torch.randn(V, De, generator=g), W=torch.randn(K, De, generator=g) * 0.3,
             b=torch.randn(De, generator=g) * 0.2, vn=torch.randn(nv, De, generator=g))
    ff = None
    if F:
        ff = torch.rand(B, N, N, F, generator=g); ff[adj == 0] = -1.0
        p.update(We=torch.randn(F, De, generator=g), be=torch.randn(De, generator=g) * 0.2)
    return adj, fm, ff, p


def _run_embed(adj, fm, ff, p, gpu, edge_dtype, vn=True):
    from egt_amd import edge_embed
    q = {k: v.to(gpu).requires_grad_() for k, v in p.items()}
    kw = {} if ff is None else dict(float_features=ff.to(gpu), float_kernel=q["We"], float_bias=q["be"])
    e = edge_embed(fm.to(gpu), adj.to(gpu), q["table"], q["W"], q["b"], edge_dtype=edge_dtype,
                   virtual_edge_table=q["vn"] if vn else None, **kw)
    return e, q


@pytest.mark.parametrize("edge_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nv,De,F", [(1, 8, 0), (3, 8, 0), (1, 64, 0), (3, 64, 0), (3, 8, 1)])
def test_bordered_embedding_forward_is_the_plain_one_plus_the_border(nv, De, F, edge_dtype, gpu, egt_lib):
    """N' = 20 / 22 straddles a 16-row tile; at nv = 1 the interior pitch is no multiple of 4.  Interior: the bits of the plain
    embedding (same table + FMA chain).  Border: the table rows / the fp32 box, rounded once in bf16."""
    B, N, K = 2, 19, 4
    adj, fm, ff, p = _embed_inputs(B, N, De, K, nv, F, seed=nv * 100 + De + F)
    e, q = _run_embed(adj, fm, ff, p, gpu, edge_dtype)
    e0, _ = _run_embed(adj, fm, ff, p, gpu, edge_dtype, vn=False)
    dt = DT[edge_dtype]
    assert e.shape == (B, nv + N, nv + N, De) and e.dtype == dt and e0.shape == (B, N, N, De)
    assert torch.equal(e[:, nv:, nv:], e0), "interior"
    vn = q["vn"].detach()
    rows = vn.to(dt)[None, :, None, :].expand(B, nv, N, De)
    assert torch.equal(e[:, :nv, nv:], rows), "virtual rows (padded columns included)"
    assert torch.equal(e[:, nv:, :nv], vn.to(dt)[None, None, :, :].expand(B, N, nv, De)), "virtual columns"
    box = (0.5 * (vn[:, None, :] + vn[None, :, :])).to(dt)
    assert torch.equal(e[:, :nv, :nv], box[None].expand(B, nv, nv, De)), "corner box"
    if edge_dtype == "f32":
        p64 = {k: v.double() for k, v in p.items()}
        ref = VR.embed_ref(fm, adj, p64["table"], p64["W"], p64["b"], p64["vn"], K, ff, p64.get("We"), p64.get("be"))
        assert_close(e, ref, name="bordered e", **FWD)


@pytest.mark.parametrize("edge_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("De", [8, 64])
def test_bordered_embedding_backward(De, edge_dtype, gpu, egt_lib):
    """B N N = 4107 pairs: three 2048-pair workgroups, so the partial reduce runs.  All four gradients against the fp64
    restatement (in bf16 it is fed the rounded d_e), two runs bit-equal, and a d_e that lives in the box alone gives the box
    term alone (a dropped 1/2 or a missing transpose term shows here)."""
    B, N, K, nv = 3, 37, 4, 2
    adj, fm, ff, p = _embed_inputs(B, N, De, K, nv, 0, seed=De)
    g = torch.Generator().manual_seed(5 + De)
    de = torch.randn(B, nv + N, nv + N, De, generator=g).to(DT[edge_dtype])
    names = ("table", "W", "b", "vn")

    def grads(d):
        e, q = _run_embed(adj, fm, ff, p, gpu, edge_dtype)
        e.backward(d.to(gpu))
        assert q["vn"].grad.dtype == torch.float32
        return [q[k].grad for k in names]
    got, again = grads(de), grads(de)
    for k, a, b in zip(names, got, again):
        assert torch.equal(a, b), f"d {k}: two runs differ"
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    ref = VR.embed_ref(fm, adj, p64["table"], p64["W"], p64["b"], p64["vn"], K)
    gr = torch.autograd.grad(ref, [p64[k] for k in names], de.double())
    for k, a, r in zip(names, got, gr):
        assert_close(a, r, name=f"d {k}", **BWD)
    box = torch.zeros_like(de)
    box[:, :nv, :nv] = de[:, :nv, :nv]
    dvn = grads(box)[3]
    d64 = box.double()[:, :nv, :nv]
    want = 0.5 * (d64.sum(dim=(0, 2)) + d64.sum(dim=(0, 1)))
    assert_close(dvn, want, name="d vn (box only)", **BWD)


@pytest.mark.parametrize("edge_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("F", [0, 1])
@pytest.mark.parametrize("De", [8, 48])
@pytest.mark.parametrize("nv", [1, 3])
def test_bordered_backward_is_the_plain_backward_of_the_interior(nv, De, F, edge_dtype, gpu, egt_lib):
    """the gradients of table, W and b (and of the feature Dense) from the bordered d_e are, bit for bit, those of the plain
    embedding from d_e[:, nv:, nv:]: both kernels walk the pairs in one order.  B N N = 2250 pairs: the second 2048-pair workgroup
    starts mid-row (graph 81, row 4, column 3).  N = 5 is below the pair lanes at either width (128 at De = 8, 16 at De = 48):
    one step of the row walk crosses several rows, at De = 8 several graphs.  De = 48: 12 quads on 16 quad lanes, so idle lanes
    meet the bordered walk.  F = 0: a table of 5 rows; F = 1: one row and one real-valued feature plane."""
    B, N, K = 90, 5, 4
    adj, fm, ff, p = _embed_inputs(B, N, De, K, nv, F, seed=1000 + nv * 100 + De + F)
    g = torch.Generator().manual_seed(7 + De + nv)
    de = torch.randn(B, nv + N, nv + N, De, generator=g).to(DT[edge_dtype])
    names = [k for k in p if k != "vn"]
    e, q = _run_embed(adj, fm, ff, p, gpu, edge_dtype)
    e.backward(de.to(gpu))
    e0, q0 = _run_embed(adj, fm, ff, p, gpu, edge_dtype, vn=False)
    e0.backward(de[:, nv:, nv:].contiguous().to(gpu))
    for k in names:
        assert torch.equal(q[k].grad, q0[k].grad), f"d {k}: bordered and plain differ"
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    ref = VR.embed_ref(fm, adj, p64["table"], p64["W"], p64["b"], p64["vn"], K, ff, p64.get("We"), p64.get("be"))
    gr = torch.autograd.grad(ref, [p64[k] for k in names], de.double())
    for k, r in zip(names, gr):
        assert_close(q[k].grad, r, name=f"d {k}", **BWD)


# ------------------------------------------------------------------------------------------------- models -----
MODEL_CASES = {   # kind, model_width, edge_width, model_height, nv, edge_channel_type, edge_dtype, N, node counts
    "zinc_w48_nv2": ("zinc", 48, 48, 2, 2, "residual", "f32", 12, (9, 5, 12)),
    "zinc_constrained_nv1": ("zinc", 64, 64, 1, 1, "constrained", "f32", 12, (9, 5, 12)),
    # (at height 1 the virtual node's prediction never sees the mask between real nodes: a second layer makes it count)
    "zinc_constrained_nv1_h2": ("zinc", 64, 64, 2, 1, "constrained", "f32", 12, (9, 5, 12)),
    "cifar10_de8_nv1": ("cifar10", 64, 8, 2, 1, "residual", "f32", 18, (18, 11, 15)),
    "cifar10_de8_nv1_bf16": ("cifar10", 64, 8, 2, 1, "residual", "bf16", 18, (18, 11, 15)),
    "zinc_bias_de8_nv1": ("zinc", 64, 8, 2, 1, "bias", "f32", 12, (9, 5, 12)),
}


def _build(case, gpu):
    from egt_amd import ZincDCTransformer, Cifar10DCTransformer
    kind, Dh, De, Ly, nv, ect, edt, N, counts = MODEL_CASES[case]
    cfg = dict(model_width=Dh, edge_width=De, model_height=Ly, upto_hop=4, edge_channel_type=ect,
               num_targets=10 if kind == "cifar10" else 1)
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    inp = VR.graphs(kind, len(counts), N, list(counts), g)
    params = VR.init_params(kind, cfg, nv, g)
    cls = Cifar10DCTransformer if kind == "cifar10" else ZincDCTransformer
    model = cls(model_width=Dh, edge_width=De, model_height=Ly, upto_hop=4, edge_channel_type=ect, num_virtual_nodes=nv,
                random_mask_prob=0.0, edge_dtype=edt).to(gpu).eval()
    loaded = set()
    with torch.no_grad():
        for k, v in params.items():
            prm = VR.module_param(model, k)
            if prm is not None:
                prm.copy_(v); loaded.add(id(prm))
    assert {id(v) for v in model.keras_named_parameters().values()} <= loaded, "a named parameter the restatement does not know"
    return model, inp, params, cfg


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_virtual_node_models_vs_restatement(case, gpu, egt_lib):
    """prediction and EVERY named parameter's gradient (the two virtual tables included) against the fp64 restatement; every
    block on the fused route.  'constrained': the mask is zero between real non-neighbours and one to and from the virtual
    node.  CIFAR10: the De = 8 kernels at odd N' = 19.  'bias': the stack reports the static-edge route."""
    from egt_amd import mae_loss, sparse_xent_loss
    from oracle import egt_model_oracle as MO
    kind, Dh, De, Ly, nv, ect, edt, N, counts = MODEL_CASES[case]
    model, inp, params, cfg = _build(case, gpu)
    dev = lambda k: inp[k].to(gpu)
    y = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    yo = VR.forward(kind, inp, p64, cfg, nv)
    if kind == "cifar10":
        loss, loss_o = sparse_xent_loss(y, dev("target")), MO.sparse_xent_loss(yo, inp["target"])
    else:
        loss, loss_o = mae_loss(y, dev("target")), MO.mae_loss(yo, inp["target"].double())
    loss.backward()
    assert [b.last_path for b in model.layers.blocks] == ["fused"] * Ly
    if ect == "bias":
        assert model.layers.last_edge_route == "static"
    if ect == "constrained":
        M = model.edge_mask(dev("graph_matrix"), None)
        assert M.shape == (len(counts), nv + N, nv + N, 8)
        assert float(M[:, :nv].min()) == 1.0 and float(M[:, :, :nv].min()) == 1.0 and float(M[:, nv:, nv:].min()) == 0.0
    tol, ptol = (FWD, BWD) if edt == "f32" else (bf16_stack_tol(2), dict(bf16_stack_tol(2, params=True), zero_atol=2e-4))
    assert_close(y, yo, name="prediction", **tol)
    gro = dict(zip(p64, torch.autograd.grad(loss_o, list(p64.values()), allow_unused=True)))
    named = model.keras_named_parameters()
    live = {id(v) for v in named.values()}
    checked = 0
    for k, gref in gro.items():
        prm = VR.module_param(model, k)
        if prm is None or id(prm) not in live:
            continue
        assert gref is not None, k
        assert_close(prm.grad, gref, name=k, **ptol); checked += 1
    assert checked == len(named)
    assert float(model.virtual_node_emb.grad.abs().max()) > 0 and float(model.virtual_edge_emb.grad.abs().max()) > 0


def test_padding_is_invisible_and_the_virtual_node_is_not(gpu, egt_lib):
    """permuting the PADDED real nodes of one graph (their features and their rows / columns of the pair inputs) leaves the
    prediction unchanged; changing virtual_node_embeddings[0] changes it"""
    model, inp, params, cfg = _build("zinc_w48_nv2", gpu)
    run = lambda d: model(d["node_features"].to(gpu), d["feature_matrix"].to(gpu), d["graph_matrix"].to(gpu)).detach()
    y = run(inp)
    perm = torch.arange(12); perm[5:] = torch.tensor([11, 9, 10, 6, 8, 5, 7])       # graph 1 has 5 real nodes
    nf2 = inp["node_features"].clone()
    nf2[1] = nf2[1][perm]                                                            # (padded slots all carry -1)
    fm2, adj2 = inp["feature_matrix"].clone(), inp["graph_matrix"].clone()
    fm2[1, 6, 8] = 2; adj2[1, 9, 10] = 1.0                                           # junk between padded nodes, then permuted
    fm2[1] = fm2[1][perm][:, perm]; adj2[1] = adj2[1][perm][:, perm]
    y2 = run(dict(node_features=nf2, feature_matrix=fm2, graph_matrix=adj2))
    assert_close(y2, y, name="padding invariance", **FWD)
    with torch.no_grad():
        model.virtual_node_emb[0, ::2] += 0.5     # (not a uniform shift of the row: every LayerNorm on the way removes one)
    assert float((run(inp) - y).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------- driver -----
def _zinc_store(tmp_path, n_train, n_val, seed=0):
    """a small packed ZINC store written through egt_amd.data: chain graphs of 5..12 nodes, symmetric edges"""
    from egt_amd import data as D
    rng = np.random.default_rng(seed)

    def records(n):
        recs = []
        for _ in range(n):
            k = int(rng.integers(5, 13))
            src = np.arange(k - 1); dst = src + 1
            edges = np.concatenate([np.stack([src, dst], 1), np.stack([dst, src], 1)]).astype(np.int32)
            ef = rng.integers(0, 3, size=k - 1).astype(np.int32)
            nf = rng.integers(0, 28, size=k).astype(np.int32)
            recs.append(dict(num_nodes=np.int32(k), edges=edges, node_features=nf, edge_features=np.concatenate([ef, ef]),
                             target=np.asarray([np.float32(nf.sum() / 100.0)])))
        return recs
    spec = D.SPECS["zinc"]
    path = str(tmp_path / "zinc.npz")
    D.write_packed_store(path, spec.db_name, dict(training=records(n_train), validation=records(n_val)),
                         {f.name: f.key for f in spec.fields}, meta=dict(num_graphs=n_train + n_val))
    return path


def test_zinc_scheme_trains_resumes_and_graphs_with_a_virtual_node(tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    store = _zinc_store(tmp_path, n_train=32, n_val=16)
    cfg = dict(scheme="zinc.svd", model_name="v", num_epochs=2, initial_lr=2e-3, batch_size=16, use_svd=False, model_width=16,
               edge_width=16, model_height=1, upto_hop=4, random_mask_prob=0.0, num_virtual_nodes=1, dataset_path=store,
               save_path=str(tmp_path / "run"))
    quiet = lambda *a: None
    torch.manual_seed(0)
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=quiet)
    s.config_summary(); s.save_config_file(); s.load_data(); s.load_model()
    init = [s.model.virtual_node_emb.detach().clone(), s.model.virtual_edge_emb.detach().clone()]
    s.load_state(); s.train_model(); s.finalize_training()
    assert s.state.current_epoch == 2 and all(math.isfinite(h["loss"]) and math.isfinite(h["val_mae"]) for h in s.history)
    assert not torch.equal(s.model.virtual_node_emb, init[0]) and not torch.equal(s.model.virtual_edge_emb, init[1])
    w = np.load(tmp_path / "run" / "saved" / "v.npz")
    assert w["virtual_node_embedding/virtual_node_embeddings"].shape == (1, 16)
    assert w["virtual_edge_embedding/virtual_edge_embeddings"].shape == (1, 16) and w["mlp_out_0/kernel"].shape == (16, 8)
    ev = T.ZincSVDScheme(cfg, device=gpu, print_fn=quiet)                           # --evaluate: the saved weights, two splits
    ev.do_evaluations(s.trainset, s.valset)
    assert open(tmp_path / "run" / "predictions" / "valset_evals.txt").read().startswith("valset MAE = ")
    s2 = T.ZincSVDScheme(dict(cfg, num_epochs=3), device=gpu, print_fn=quiet)
    s2.load_data(); s2.load_model(); s2.load_state()
    assert s2.state.current_epoch == 2
    assert torch.equal(s2.model.virtual_node_emb, s.model.virtual_node_emb)
    assert torch.equal(s2.model.virtual_edge_emb, s.model.virtual_edge_emb)
    batch = next(iter(s.valset))

    def one_step(tag, graph):
        torch.manual_seed(1)
        t = T.ZincSVDScheme(dict(cfg, model_name=tag, use_hipgraph=graph, save_path=str(tmp_path / tag)), device=gpu, print_fn=quiet)
        t.load_model()
        return t.train_step(batch), [p.detach().clone() for p in t.params]
    (le, pe), (lg, pg) = one_step("e", False), one_step("g", True)
    assert le == lg
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
