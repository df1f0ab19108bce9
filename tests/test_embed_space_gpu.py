"""The edge embedding across its instance table and its widths, against fp64 autograd of the restatement
(O.dense(MO.stack_hops) + MO.neg1_masked_embedding [+ Dense(keras_masking)], virtual_nodes_ref.embed_ref for the bordered form).

Instance table: the backward is k_edge_embed_bwd<K_, V_, T, VN>, K_ = upto_hop + num_float_features in 1..20 planes, V_ =
num_edge_features + 1 in 1..8 table rows, T fp32 / bf16 storage, plain / bordered -- 640 instances picked by two macro-built
switches.  Every one runs here, at B = 2, N = 9 and at B = 2, N = 33 (two backward workgroups): upto_hop = min(K_, 16) and F = K_ - upto_hop real-valued features (K_ = 17..20:
F = 1..4); every table row selected by some pair, the -1 row included.  The four test functions loop over the 160 (K_, V_) pairs
and report the pairs that failed together, so a wrong `case` line reads as the set of pairs that went through it.

Widths: every edge width 4, 8, .., 64 the embedding accepts at B = 3, N = 37 (4107 pairs: three backward workgroups, so the
reduction over the partials runs), K = 4, V = 5; plain, nv = 1 and nv = 3.  The widths whose De / 4 is no power of two leave lanes
of the backward and of k_edge_embed_vn_border_bwd idle (c4 >= C4).

Feature ids stay inside -1..V-2: the kernels clamp what lies outside, and the reference defines nothing there."""
import pytest
import torch

import virtual_nodes_ref as VR
from test_bf16_edges_gpu import check_stored
from util import assert_close, FWD, BWD

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAMES = ("d fm_table", "d adj_emb.kernel", "d adj_emb.bias", "d edge_emb.kernel", "d edge_emb.bias", "d vn_table")


def _path(N):
    a = torch.zeros(N, N)
    i = torch.arange(N - 1)
    a[i, i + 1] = 1.0; a[i + 1, i] = 1.0
    return a


def _graphs(B, N, g):
    """graph 0 a path over all N nodes (its hop planes differ from one another until the walk spans it), the others random and
    symmetric with about 3 neighbours per node, the last one padded by two nodes"""
    adj = (torch.rand(B, N, N, generator=g) < 1.5 / N).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float()
    adj[0] = _path(N)
    adj[B - 1, N - 2:, :] = 0.0; adj[B - 1, :, N - 2:] = 0.0
    return adj


def _inputs(K_, V_, De, B, N, nv, dtype):
    upto, F = min(K_, 16), K_ - min(K_, 16)
    g = torch.Generator().manual_seed(100000 * nv + 1000 * De + 10 * K_ + V_)
    adj = _graphs(B, N, g)
    fm = (torch.arange(B * N * N) % V_ - 1)[torch.randperm(B * N * N, generator=g)].reshape(B, N, N)   # every row, -1 among them
    ff = None
    if F:
        ff = torch.rand(B, N, N, F, generator=g)
        ff[torch.rand(B, N, N, generator=g) < 0.3] = -1.0             # masked pairs: every feature at the mask value
        ff[0, 0, 1] = -1.0; ff[0, 0, 1, F - 1] = 0.5                  # one differing feature keeps the pair
    p = dict(table=torch.randn(V_, De, generator=g), W=torch.randn(upto, De, generator=g) * 0.3, b=torch.randn(De, generator=g) * 0.2)
    if F:
        p.update(We=torch.randn(F, De, generator=g) * 0.5, be=torch.randn(De, generator=g) * 0.1)
    if nv:
        p.update(vn=torch.rand(nv, De, generator=g) * 2 - 1)
    de = torch.randn(B, nv + N, nv + N, De, generator=g)
    if dtype == "bf16":
        de = de.to(BF)                                                # the oracle is fed the rounded d_e
    return upto, adj, fm, ff, p, de


def _oracle(upto, adj, fm, ff, p, de):
    from oracle import egt_model_oracle as MO, egt_oracle as O
    q = {k: v.double().requires_grad_() for k, v in p.items()}
    if "vn" in q:
        e = VR.embed_ref(fm, adj, q["table"], q["W"], q["b"], q["vn"], upto, ff, q.get("We"), q.get("be"))
    else:
        e = O.dense(MO.stack_hops(adj.double(), upto), q["W"], q["b"]) + MO.neg1_masked_embedding(fm, q["table"])
        if ff is not None:
            xe, _ = MO.keras_masking(ff.double(), -1.0)
            e = e + O.dense(xe, q["We"], q["be"])
    return e.detach(), dict(zip(q, torch.autograd.grad(e, list(q.values()), de.double())))


def _run(gpu, adj, fm, ff, p, de, dtype):
    from egt_amd import edge_embed
    q = {k: v.to(gpu).requires_grad_() for k, v in p.items()}
    kw = {} if ff is None else dict(float_features=ff.to(gpu), float_kernel=q["We"], float_bias=q["be"], mask_value=-1.0)
    e = edge_embed(fm.to(gpu), adj.to(gpu), q["table"], q["W"], q["b"], edge_dtype=dtype, virtual_edge_table=q.get("vn"), **kw)
    e.backward(de.to(gpu))
    return e.detach(), {k: v.grad for k, v in q.items()}


# (2, 9): one backward workgroup.  (2, 33): 2178 pairs, two workgroups -- an instance with MORE table rows than the descriptor
# writes the rows the reduction reads when there is one partial (the rows sit at the front of it); only the stride between two
# partials tells it from the right one.
INSTANCE_SHAPES = ((2, 9), (2, 33))
GRAD_NAME = dict(table=NAMES[0], W=NAMES[1], b=NAMES[2], We=NAMES[3], be=NAMES[4], vn=NAMES[5])


def _compare(gpu, K_, V_, De, B, N, nv, dtype, twice=False):
    upto, adj, fm, ff, p, de = _inputs(K_, V_, De, B, N, nv, dtype)
    e_o, gr = _oracle(upto, adj, fm, ff, p, de)
    e, grads = _run(gpu, adj, fm, ff, p, de, dtype)
    tag = f"K_={K_} V_={V_} De={De} nv={nv} {dtype}"
    assert e.shape == (B, nv + N, nv + N, De)
    if dtype == "bf16":
        check_stored(e, e_o, name=f"e0 [{tag}]", **FWD)
    else:
        assert e.dtype == torch.float32
        assert_close(e, e_o, name=f"e0 [{tag}]", **FWD)
    for k, gref in gr.items():
        assert grads[k].dtype == torch.float32
        assert_close(grads[k], gref, name=f"{GRAD_NAME[k]} [{tag}]", **BWD)
    if twice:
        e2, grads2 = _run(gpu, adj, fm, ff, p, de, dtype)
        assert torch.equal(e, e2), f"e0 is not bit-reproducible [{tag}]"
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), f"{GRAD_NAME[k]} is not bit-reproducible [{tag}]"


@pytest.mark.parametrize("nv", [0, 1], ids=["plain", "bordered"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_backward_instance_vs_oracle(dtype, nv, gpu, egt_lib):
    failed = []
    for K_ in range(1, 21):
        for V_ in range(1, 9):
            try:
                for B, N in INSTANCE_SHAPES:
                    _compare(gpu, K_, V_, 8, B, N, nv, dtype)
            except AssertionError as ex:
                failed.append(((K_, V_), str(ex).splitlines()[0][:200]))
    assert not failed, (f"{len(failed)} of 160 (K_, V_) instances differ from the oracle: {[kv for kv, _ in failed]}; first: "
                        f"{failed[0][1]}")


@pytest.mark.parametrize("nv", [0, 1, 3], ids=["plain", "nv1", "nv3"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_edge_width_vs_oracle(dtype, nv, gpu, egt_lib):
    failed = []
    for De in range(4, 68, 4):
        try:
            _compare(gpu, 4, 5, De, 3, 37, nv, dtype, twice=True)
        except AssertionError as ex:
            failed.append((De, str(ex).splitlines()[0][:200]))
    assert not failed, f"{len(failed)} of 16 widths differ from the oracle: {[w for w, _ in failed]}; first: {failed[0][1]}"
