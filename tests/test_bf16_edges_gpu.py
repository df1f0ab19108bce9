"""bf16 edge tensors end to end (include/egt_amd.h EGT_BF16) on the MI355X: the channel FFN and the edge embedding with bf16
storage against fp64 oracles, EGTLayerStack and the CIFAR10 model (BASELINE config 3 as specified) in bf16, and the training
driver's edge_dtype key.

Tolerance model of a single operator with bf16 storage: the oracle reads the SAME bf16 inputs (exact values) and rounds its
outputs to bf16 where the kernel stores them.  fp32 outputs (parameter gradients) keep the fp32 tolerances (util.FWD / BWD).
A stored bf16 element must equal the oracle's rounded value, with ONE allowance: where the exact value lies within the fp32
tolerance of a bf16 rounding boundary, the kernel's fp32 value may round to a neighbouring bf16 value.  Put exactly: the
stored value must be the round-to-nearest-even image of SOME value within the fp32 tolerance of the oracle (one bf16 ulp
for every element whose fp32 tolerance is narrower than a bf16 ulp -- all but the elements near zero, where the absolute
term arel * max|ref| dominates)."""
import math

import pytest
import torch

from util import assert_close, margin, bf16_stack_tol, FWD, BWD
from test_block_gpu import _Bf16Storage, PMAP
from test_model import _load_params, _grad_of

pytestmark = pytest.mark.gpu

NAMES = ("norm_gamma", "norm_beta", "lr1_kernel", "lr1_bias", "lr2_kernel", "lr2_bias")
BF = torch.bfloat16


def check_stored(actual, ref, *, rtol, arel, name, l2=None, **_):
    """actual: a bf16 tensor the kernel stored; ref: the fp64 oracle value before the store's rounding."""
    assert actual.dtype == BF, f"{name}: stored as {actual.dtype}"
    a = actual.detach().double().cpu(); r = ref.detach().double().cpu()
    assert a.shape == r.shape and torch.isfinite(a).all(), name
    rb = r.to(BF).double()
    tol = arel * float(r.abs().max()) + rtol * r.abs()
    lo, hi = (r - tol).to(BF).double(), (r + tol).to(BF).double()      # every bf16 value an fp32 result within tol rounds to
    ok = (a == rb) | ((a >= lo) & (a <= hi))
    if not ok.all():
        bad = int((~ok).sum())
        raise AssertionError(f"{name}: {bad}/{a.numel()} stored elements are not the rounding of a value within the fp32 "
                             f"tolerance (e.g. flat index {int((~ok).flatten().nonzero()[0])}: got "
                             f"{float(a.flatten()[(~ok).flatten()][0]):.6e}, oracle {float(r.flatten()[(~ok).flatten()][0]):.9e})")
    if rtol < 2 ** -9:   # the fp32 tolerance is narrower than half a bf16 ulp: off-by-one stores are the exception
        off = float((a != rb).double().mean())
        assert off < 0.02, f"{name}: {off:.3%} of the stored elements sit one ulp off the rounded oracle"


# ------------------------------------------------------------------------------------------------------ channel FFN --
def _ffn_once(m, x, dy):
    xg = x.clone().requires_grad_()
    for p in m.parameters():
        p.grad = None
    y = m(xg)
    y.backward(dy)
    return y.detach(), xg.grad.detach(), [getattr(m, n).grad.detach().clone() for n in NAMES]


CASES = [(8, "f32", (2, 37, 37), "elu"), (8, "f32", (3, 17, 17), "relu"), (8, "f32", (1, 63), "elu"), (8, "f32", (4, 150, 150), "elu")]
for _W, _shape in ((16, (2, 23, 23)), (32, (2, 19, 19)), (48, (2, 21, 21)), (64, (2, 24, 24)), (64, (1, 5))):
    for _mm in ("f32", "bf16x3", "bf16"):
        # (relu at width 32; not with plain bf16 products, whose 2e-2 errors flip relu's step for pre-activations near 0 --
        #  tests/test_ffn_gpu.py runs that mode on elu too)
        CASES.append((_W, _mm, _shape, "relu" if _W == 32 and _mm != "bf16" else "elu"))


@pytest.mark.parametrize("W,matmul,shape,act", CASES)
def test_ffn_bf16_storage_vs_oracle(W, matmul, shape, act, gpu, egt_lib):
    """x, y, dy, dx in bf16; the six parameter gradients fp32.  Width 8 at an odd row count (1 x 63) and at config 3's
    [4,150,150]; ragged tile counts at the tile widths; every product mode each width takes."""
    from egt_amd import FFN
    from oracle import egt_oracle as O
    torch.manual_seed(W + len(shape))
    m = FFN(W, activation=act, matmul=matmul).to(gpu)
    with torch.no_grad():
        for n in ("norm_gamma", "norm_beta", "lr1_bias", "lr2_bias"):
            getattr(m, n).add_(0.3 * torch.randn_like(getattr(m, n)))
    g = torch.Generator().manual_seed(7 * W + 1)
    x = (torch.randn(*shape, W, generator=g) * 1.5 + 0.2).to(BF)
    dy = torch.randn(*shape, W, generator=g).to(BF)
    y, dx, grads = _ffn_once(m, x.to(gpu), dy.to(gpu))
    assert y.dtype == BF and dx.dtype == BF and all(t.dtype == torch.float32 for t in grads)
    y2, dx2, grads2 = _ffn_once(m, x.to(gpu), dy.to(gpu))
    assert torch.equal(y, y2) and torch.equal(dx, dx2), "bf16 FFN is not bit-reproducible"
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b), "bf16 FFN parameter gradients are not bit-reproducible"
    p64 = {n: getattr(m, n).detach().double().cpu().requires_grad_() for n in NAMES}
    x64 = x.double().requires_grad_()
    yo = O.ffn_forward(x64, p64, activation=act)
    gr = torch.autograd.grad(yo, [x64] + [p64[n] for n in NAMES], dy.double())
    fwd, bwd = (FWD, BWD) if matmul != "bf16" else (dict(rtol=2e-2, arel=1e-2, l2=2e-2),) * 2
    check_stored(y, yo, name="y", **fwd)
    check_stored(dx, gr[0], name="dx", **bwd)
    for n, a, gref in zip(NAMES, grads, gr[1:]):
        assert_close(a, gref, name="d" + n, **bwd)


def test_ffn_bf16_dx_may_alias_dy(gpu, egt_lib):
    """the C-ABI contract: dx may alias dy (in bf16 too)"""
    import ctypes as C
    from egt_amd import FFN, _lib as L
    from egt_amd.ffn import _desc, _pstruct
    for W, rows in ((8, 1001), (64, 333)):
        m = FFN(W).to(gpu)
        g = torch.Generator().manual_seed(W)
        x = torch.randn(rows, W, generator=g).to(BF).to(gpu)
        dy = torch.randn(rows, W, generator=g).to(BF).to(gpu)
        lib = L.load()
        d = _desc(rows, W, "elu", 1e-3, "f32", BF)
        ws = torch.empty(lib.egt_ffn_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=gpu)
        ps = _pstruct([getattr(m, n).detach() for n in NAMES])
        outs = []
        for alias in (False, True):
            gs = [torch.empty_like(getattr(m, n)) for n in NAMES]
            dyc = dy.clone()
            dx = dyc if alias else torch.empty_like(dy)
            L.check(lib.egt_ffn_bwd(C.byref(d), C.byref(ps), L.ptr(x), L.ptr(dyc), L.ptr(dx), C.byref(_pstruct(gs)), L.ptr(ws),
                                    L.current_stream()))
            outs.append((dx.clone(), gs))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0])
        for a, b in zip(outs[0][1], outs[1][1]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- edge embedding --
@pytest.mark.parametrize("form,B,N,De,K", [("zinc", 2, 37, 64, 16), ("zinc", 3, 21, 8, 4), ("cifar10", 2, 150, 8, 4),
                                           ("cifar10", 2, 33, 16, 3)])
def test_edge_embed_bf16_vs_oracle(form, B, N, De, K, gpu, egt_lib):
    """ZINC form (integer feature table) and CIFAR10 form (real-valued feature plane through Masking + Dense): e0 stored
    in bf16, its gradient read in bf16, every parameter gradient fp32."""
    from egt_amd import edge_embed
    from oracle import egt_model_oracle as MO, egt_oracle as O
    g = torch.Generator().manual_seed(B * 1000 + N + De)
    adj = (torch.rand(B, N, N, generator=g) > 0.8).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float()
    V = 5 if form == "zinc" else 1
    W = torch.randn(K, De, generator=g) * 0.3; b = torch.randn(De, generator=g) * 0.2
    de = torch.randn(B, N, N, De, generator=g).to(BF)
    if form == "zinc":
        fm = torch.where(adj > 0, torch.randint(0, V - 1, (B, N, N), generator=g), torch.tensor(-1))
        table = torch.randn(V, De, generator=g)
        ff = fk = fb = None
    else:
        fm = torch.full((B, N, N), -1, dtype=torch.int32)
        table = torch.zeros(1, De)
        ff = torch.rand(B, N, N, 1, generator=g); ff[adj == 0] = -1.0
        fk = torch.randn(1, De, generator=g) * 0.5; fb = torch.randn(De, generator=g) * 0.1
    ps = [table, W, b] + ([] if ff is None else [fk, fb])
    p64 = [x.double().requires_grad_() for x in ps]
    e_o = O.dense(MO.stack_hops(adj.double(), K), p64[1], p64[2]) + MO.neg1_masked_embedding(fm, p64[0])
    if ff is not None:
        xe, _ = MO.keras_masking(ff.double(), -1.0)
        e_o = e_o + O.dense(xe, p64[3], p64[4])
    gr = torch.autograd.grad(e_o, p64, de.double())
    pg = [x.to(gpu).requires_grad_() for x in ps]
    kw = {} if ff is None else dict(float_features=ff.to(gpu), float_kernel=pg[3], float_bias=pg[4], mask_value=-1.0)
    e = edge_embed(fm.to(gpu), adj.to(gpu), pg[0], pg[1], pg[2], edge_dtype="bf16", **kw)
    check_stored(e, e_o, name="e0", **FWD)
    e.backward(de.to(gpu))
    # two runs match bitwise: e0 and every parameter gradient
    g1 = [None if p.grad is None else p.grad.clone() for p in pg]
    for p in pg:
        p.grad = None
    e2 = edge_embed(fm.to(gpu), adj.to(gpu), pg[0], pg[1], pg[2], edge_dtype="bf16", **kw)
    e2.backward(de.to(gpu))
    assert torch.equal(e.detach(), e2.detach()), "bf16 edge embedding is not bit-reproducible"
    for a, p in zip(g1, pg):
        assert (a is None and p.grad is None) or torch.equal(a, p.grad), "bf16 embedding gradients are not bit-reproducible"
    names = ["d fm_emb", "d adj_emb.kernel", "d adj_emb.bias", "d edge_emb.kernel", "d edge_emb.bias"]
    for i, (p, gref) in enumerate(zip(pg, gr)):
        if form == "cifar10" and i == 0:
            continue   # the constant one-row zero table of the CIFAR10 model (a buffer, not a parameter)
        assert p.grad.dtype == torch.float32
        assert_close(p.grad, gref, name=names[i], **BWD)
    # fp32 storage of the same call is unchanged: e0 rounds to the bf16 result
    e32 = edge_embed(fm.to(gpu), adj.to(gpu), pg[0], pg[1], pg[2], **kw)
    assert e32.dtype == torch.float32 and torch.equal(e32.detach().to(BF), e.detach())


# ----------------------------------------------------------------------------------------------------- layer stack --
@pytest.mark.parametrize("N,De,overlap", [(23, 8, False), (40, 8, True), (32, 64, False), (19, 64, True)])
def test_layer_stack_bf16_vs_both_oracles(N, De, overlap, gpu, egt_lib, capsys):
    """EGTLayerStack (attention block, then both FFNs, Ly = 2) with bf16 e.  Storage points on the edge path: per layer the
    block's e' and the FFN's e'' in the forward and their two gradients in the backward -- 4 per layer, 8 in all.
    (a) the oracle that rounds e at those points, under the single-operator bf16 tolerance (bf16_stack_tol(1));
    (b) the plain fp64 oracle under the square-root depth rule of tests/util.py, whose unit is a pair of storage points
    (one forward, one backward): 8 points = bf16_stack_tol(4)."""
    from egt_amd import EGTLayerStack
    from oracle import egt_oracle as O
    torch.manual_seed(17 + De)   # (worst margins printed below: h / e outputs and parameter gradients)
    B, Ly = 2, 2
    st = EGTLayerStack(model_height=Ly, model_width=64, edge_width=De, num_heads=8, fused=True).to(gpu).eval()
    st.check_edge_dtype(BF)
    st.overlap_ffn = overlap
    with torch.no_grad():
        for prm in st.parameters():
            if prm.dim() == 1:
                prm.add_(0.2 * torch.randn_like(prm))
    g = torch.Generator().manual_seed(3 + N)
    h = torch.randn(B, N, 64, generator=g); e = torch.randn(B, N, N, De, generator=g).to(BF)
    mask = torch.ones(B, N, dtype=torch.bool); mask[0, N - 4:] = False
    dh = torch.randn(B, N, 64, generator=g); de = torch.randn(B, N, N, De, generator=g).to(BF)
    hg = h.to(gpu).requires_grad_(); eg = e.to(gpu).requires_grad_()
    h2, e2 = st(hg, eg, mask.to(gpu))
    assert e2.dtype == BF and h2.dtype == torch.float32
    assert all(b.last_path in ("fused",) for b in st.blocks)
    torch.autograd.backward([h2, e2], [dh.to(gpu), de.to(gpu)])
    assert eg.grad.dtype == BF

    def oracle(storage):
        S = _Bf16Storage.apply if storage else (lambda t: t)
        layers = [{k: getattr(getattr(blk, m), a_).detach().double().cpu().requires_grad_() for k, (m, a_) in PMAP.items()}
                  for blk in st.blocks]
        fe = [{n: getattr(st.ffn_edge[i], n).detach().double().cpu().requires_grad_() for n in NAMES} for i in range(Ly)]
        fn = [{n: getattr(st.ffn_node[i], n).detach().double().cpu().requires_grad_() for n in NAMES} for i in range(Ly)]
        h64 = h.double().requires_grad_(); e64 = e.double().requires_grad_()
        ho, eo = h64, e64
        for i in range(Ly):
            ho, eo = O.block_forward(ho, eo, mask, layers[i], num_heads=8)
            eo = S(O.ffn_forward(S(eo), fe[i]))
            ho = O.ffn_forward(ho, fn[i])
        flat = [t for i in range(Ly) for t in list(layers[i].values()) + list(fe[i].values()) + list(fn[i].values())]
        gr = torch.autograd.grad([ho, eo], [h64, e64] + flat, [dh.double(), de.double()])
        return ho, eo, gr

    mine = [t.grad for i in range(Ly) for t in
            [getattr(getattr(st.blocks[i], m), a_) for (m, a_) in PMAP.values()] + [getattr(st.ffn_edge[i], n) for n in NAMES]
            + [getattr(st.ffn_node[i], n) for n in NAMES]]
    worst = {}
    for storage, (tol, ptol) in ((True, (bf16_stack_tol(1), bf16_stack_tol(1, params=True))),
                                 (False, (bf16_stack_tol(2 * Ly), bf16_stack_tol(2 * Ly, params=True)))):
        ho, eo, gr = oracle(storage)
        de_ref = gr[1].to(BF).double() if storage else gr[1]
        tag = "storage" if storage else "plain"
        assert_close(h2, ho, name=f"h_out ({tag})", **tol)
        assert_close(e2.float(), eo, name=f"e_out ({tag})", **tol)
        assert_close(hg.grad, gr[0], name=f"dh ({tag})", **tol)
        if storage:
            assert_close(eg.grad.float(), de_ref, name=f"de ({tag})", **tol)
        else:
            # de passes back through 2 Ly LayerNorm backwards over De channels, whose 1/std amplifies the storage rounding
            # of single elements: the quadrature rule bounds its normalised L2 error (measured worst element at N = 40,
            # De = 8: 1.02 of the elementwise bound); the elementwise check of de is oracle (a)'s
            l2 = float((eg.grad.double().cpu() - de_ref).norm() / de_ref.norm())
            assert l2 <= tol["rtol"], f"de (plain): normalised L2 error {l2:.3e} > {tol['rtol']:.3e}"
        w = max(margin(a, r, **ptol) for a, r in zip(mine, gr[2:]) if a is not None and float(r.abs().max()) > 1e-9)
        assert w < 1.0, f"a parameter gradient is out of tolerance ({tag}): worst margin {w:.2f}"
        worst[tag] = max(margin(h2, ho, **tol), margin(e2.float(), eo, **tol), w)
    with capsys.disabled():
        print(f"\n[bf16 layer stack N={N} De={De}] worst error / tolerance: storage oracle {worst['storage']:.2f}, "
              f"plain oracle {worst['plain']:.2f}")


# ---------------------------------------------------------------------------------------- config 3, whole model --
def test_config3_model_bf16_vs_both_oracles(gpu, egt_lib, capsys):
    """Cifar10DCTransformer(edge_dtype="bf16") at BASELINE config 3's shapes: N = 150, Dh = 64, De = 8, H = 8, Ly = 4, in
    training mode (random_mask_prob 0.1, the per-layer masks injected into the oracle from the counter hash), node counts in
    [85, 150].  Logits, loss and every trainable parameter gradient against (a) the oracle that rounds the edge tensor where
    the model stores it, under the single-operator bf16 tolerance, and (b) the plain fp64 oracle under the depth rule.
    Storage points on the edge path: e0 of the embedding, e' of each of the 4 blocks and e'' of the 3 live edge FFNs (the last
    layer's edge FFN is not part of the model) = 8 forward + 8 gradients = 16 points = bf16_stack_tol(8)."""
    from egt_amd import Cifar10DCTransformer, sparse_xent_loss
    from oracle import egt_model_oracle as MO, egt_oracle as O, rng_ref
    B, N, Ly, p_rm = 2, 150, 4, 0.1
    cfg = dict(model_width=64, edge_width=8, model_height=Ly, upto_hop=4, num_node_features=1, num_edge_features=0,
               num_targets=10, float_node_features=5, float_edge_features=1)
    g = torch.Generator().manual_seed(150)
    n = torch.tensor([150, 85]); real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
    adj = (torch.rand(B, N, N, generator=g) > 0.92).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
    y = torch.randint(0, 10, (B,), generator=g)
    params = MO.init_zinc_params(cfg, dtype=torch.float32, generator=g)
    model = Cifar10DCTransformer(model_width=64, model_height=Ly, upto_hop=4, random_mask_prob=p_rm, seed=3,
                                 edge_dtype="bf16").to(gpu).train()
    _load_params(model, params, gpu)
    rms = []
    for blk in model.layers.blocks:
        m = blk.mha
        sd = (m.seed * 0x9E3779B97F4A7C15 + (m._calls + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        rms.append(torch.from_numpy(rng_ref.random_mask(sd, B, N, 8, p_rm)))
    logits = model(nf.to(gpu), fm.to(gpu), adj.to(gpu))
    loss = sparse_xent_loss(logits, y.to(gpu))
    loss.backward()
    assert all(b.last_path == "fused" for b in model.layers.blocks)
    dead = {id(q) for q in model._dead_edge_params()}

    def oracle(storage):
        S = _Bf16Storage.apply if storage else (lambda t: t)
        p64 = {k: v.double().requires_grad_() for k, v in params.items()}
        xn, mask = MO.keras_masking(nf.double(), -1.0)
        h = O.dense(xn, p64["node_emb.kernel"], p64["node_emb.bias"])
        xe, _ = MO.keras_masking(fm.double(), -1.0)
        e = O.dense(xe, p64["edge_emb.kernel"], p64["edge_emb.bias"])
        e = S(e + O.dense(MO.stack_hops(adj.double(), cfg["upto_hop"]), p64["adj_emb.kernel"], p64["adj_emb.bias"]))
        for ii in range(Ly):
            bp = {k[len(f"layer{ii}."):]: v for k, v in p64.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
            h, e = O.block_forward(h, e, mask, bp, num_heads=8, rand_mask=rms[ii])
            e = S(e)
            fn = {k.split(".", 2)[2]: v for k, v in p64.items() if k.startswith(f"layer{ii}.ffn_node.")}
            fe = {k.split(".", 2)[2]: v for k, v in p64.items() if k.startswith(f"layer{ii}.ffn_edge.")}
            if ii < Ly - 1:
                e = S(O.ffn_forward(e, fe))
            h = O.ffn_forward(h, fn)
        h = O.layer_norm(h, p64["node_norm_final.gamma"], p64["node_norm_final.beta"])
        x = MO.mlp_out(MO.masked_global_avg_pool_1d(h, mask), p64, 2, "elu")
        lo = O.dense(x, p64["target.kernel"], p64["target.bias"])
        lss = MO.sparse_xent_loss(lo, y)
        names = [k for k in p64 if k not in ("fm_emb.embeddings", "node_emb.embeddings")]
        gro = torch.autograd.grad(lss, [p64[k] for k in names], allow_unused=True)
        return lo, lss, dict(zip(names, gro))

    margins = {}
    for storage, (tol, ptol) in ((True, (bf16_stack_tol(1), bf16_stack_tol(1, params=True))),
                                 (False, (bf16_stack_tol(8), bf16_stack_tol(8, params=True)))):
        tag = "storage" if storage else "plain"
        lo, lss, gro = oracle(storage)
        assert_close(logits, lo, name=f"logits ({tag})", **tol)
        assert_close(loss.reshape(1), lss.reshape(1), name=f"xent ({tag})", **tol)
        worst, checked = {"logits": margin(logits, lo, **tol), "xent": margin(loss.reshape(1), lss.reshape(1), **tol)}, 0
        for k, gref in gro.items():
            if k.startswith("node_emb.") or k.startswith("edge_emb."):
                prm = getattr(getattr(model, k.split(".")[0]), k.split(".")[1])
            else:
                prm = _grad_of(model, k)
            if prm is None or id(prm) in dead or gref is None:
                continue
            if float(gref.abs().max()) > 1e-9:
                assert_close(prm.grad, gref, name=f"{k} ({tag})", **ptol)
                worst[k] = margin(prm.grad, gref, **ptol)
            checked += 1
        assert checked > 80, checked
        margins[tag] = worst
    with capsys.disabled():
        for tag, w in margins.items():
            k = max(w, key=w.get)
            print(f"\n[bf16 config 3 model, Ly = 4, N = 150] vs the {tag} oracle: logits {w['logits']:.2f}, xent {w['xent']:.2f}; "
                  f"worst of all: {k} {w[k]:.2f}")


# -------------------------------------------------------------------------------------------------- training driver --
def _cifar_cfg(tmp_path, tag, **kw):
    return dict(dict(scheme="cifar10.svd", model_name=tag, num_epochs=2, initial_lr=2e-3, batch_size=8, use_svd=False,
                     model_width=32, edge_width=8, model_height=2, upto_hop=4, random_mask_prob=0.0, edge_dtype="bf16",
                     save_path=str(tmp_path / tag)), **kw)


def test_training_driver_trains_cifar10_in_bf16(tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    tr = T.SyntheticCifar10(64, 16, nodes=(20, 44), seed=1, pad_multiple=16)
    va = T.SyntheticCifar10(32, 16, nodes=(20, 44), seed=2, pad_multiple=16)
    torch.manual_seed(0)
    s = T.Cifar10SVDScheme(_cifar_cfg(tmp_path, "b", num_epochs=3, random_mask_prob=0.1), device=gpu, print_fn=lambda *a: None)
    s.load_data(tr, va); s.load_model(); s.load_state()
    assert s.model.edge_dtype == BF
    before = [p.detach().clone() for p in s.params]
    s.train_model()
    assert all(math.isfinite(h["loss"]) for h in s.history), s.history
    assert s.history[-1]["loss"] < s.history[0]["loss"], s.history
    assert all(not torch.equal(a, b) for a, b in zip(before, s.params) if a.numel() > 1)
    # resume: a new run with one more epoch restores the checkpoint (the weights bit for bit) and continues
    s2 = T.Cifar10SVDScheme(_cifar_cfg(tmp_path, "b", num_epochs=4, random_mask_prob=0.1), device=gpu, print_fn=lambda *a: None)
    s2.load_data(tr, va); s2.load_model(); s2.load_state()
    assert s2.state.current_epoch == 3
    for a, b in zip(s.params, s2.params):
        assert torch.equal(a, b)
    s2.train_model()
    assert s2.state.current_epoch == 4 and math.isfinite(s2.history[-1]["loss"])


def test_use_hipgraph_reproduces_the_eager_bf16_run(tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    mk = lambda seed, n: T.SyntheticCifar10(n, 8, nodes=(20, 44), seed=seed, pad_multiple=1)

    def run(tag, graph, p=0.0):
        torch.manual_seed(0)
        s = T.Cifar10SVDScheme(_cifar_cfg(tmp_path, tag, use_hipgraph=graph, random_mask_prob=p), device=gpu,
                               print_fn=lambda *a: None)
        s.execute_training(mk(1, 64), mk(2, 16))
        return s
    eager, graphed = run("e", False), run("g", True)
    assert len(graphed._graphs) >= 2
    assert [h["loss"] for h in graphed.history] == [h["loss"] for h in eager.history]
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
    # with the random mask: every geometry's graph advances the shared device-resident seeds, and the run trains
    r = run("r", True, 0.1)
    assert r._seeds is not None and all(math.isfinite(h["loss"]) for h in r.history)
    assert r.history[-1]["loss"] < r.history[0]["loss"], r.history
