"""Shared inputs and the fp64 oracle of the graph-level readout head (tests/test_graph_head_*.py).  No test functions here.

The oracle is assembled from the project's existing oracle code: oracle.egt_oracle.layer_norm / dense and
oracle.egt_model_oracle.masked_global_avg_pool_1d / mlp_out / mae_loss / sparse_xent_loss."""
import zlib

import torch

from oracle import egt_oracle as O
from oracle import egt_model_oracle as MO

NAMES = ("node_norm_final.gamma", "node_norm_final.beta", "mlp_out_0.kernel", "mlp_out_0.bias", "mlp_out_1.kernel",
         "mlp_out_1.bias", "target.kernel", "target.bias")
S_UP = 0.7                                   # a non-unit upstream gradient of stats[0]
CAP = 0.25                                   # a case is admitted only if the composed fp32 head stays within CAP of the tolerance

# id -> (W, (M0, M1), loss, C, B, N, real nodes per graph (None: random 1..N), nv, activation, LayerNorm)
CASES = {
    "w64_mae_n19": (64, (32, 16), "mae", 1, 3, 19, [19, 7, 1], 0, "elu", True),          # N not a multiple of 16, a one-node graph
    "w48_mae_n37": (48, (24, 12), "mae", 1, 3, 37, [37, 9, 20], 0, "elu", True),         # idle lanes at W = 48, the ZINC-100k shape
    "w64_xent_n19": (64, (32, 16), "xent", 10, 3, 19, [19, 12, 1], 0, "elu", True),      # the classification loss and hit count
    "w64_xent_n150": (64, (32, 16), "xent", 10, 4, 150, [150, 85, 100, 1], 0, "elu", True),   # many rows per workgroup (CIFAR10's N)
    "w64_mae_1x1": (64, (32, 16), "mae", 1, 1, 1, [1], 0, "elu", True),                  # single row, single graph
    "w64_mae_b70": (64, (32, 16), "mae", 1, 70, 6, None, 0, "elu", True),                # cross-graph sums beyond one 64-graph chunk
    "w64_mae_nv1": (64, (32, 16), "mae", 1, 3, 19, [19, 8, 2], 1, "elu", True),          # virtual-node readout
    "w64_xent_nv2": (64, (32, 16), "xent", 10, 2, 19, [19, 5], 2, "elu", True),          # two virtual rows flattened
    "w48_xent_nv4": (48, (24, 12), "xent", 3, 2, 9, [9, 3], 4, "elu", True),             # widest required Dense_0 input
    "w64_mae_relu_noln": (64, (32, 16), "mae", 1, 3, 19, [19, 7, 1], 0, "relu", False),  # activation and NULL gamma / beta
}
RECIPES = ("offset32", "const_rows", "outliers")
RECIPE_CASES = ("w64_mae_n19", "w48_mae_n37", "w64_xent_n19")


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def make_case(cid, recipe="plain"):
    """-> dict(h [B,nv+N,W], mask [B,nv+N] bool, target, params (8, gamma / beta None without LayerNorm), ...)"""
    W, (M0, M1), loss, C, B, N, real, nv, act, ln = CASES[cid]
    g = gen("graph_head", cid)
    rn = lambda *s: torch.randn(*s, generator=g)
    K = max(nv, 1) * W
    params = (1.0 + 0.2 * rn(W) if ln else None, 0.2 * rn(W) if ln else None, rn(K, M0) * (1.5 / K ** 0.5), 0.2 * rn(M0),
              rn(M0, M1) * (1.5 / M0 ** 0.5), 0.2 * rn(M1), rn(M1, C) * (1.5 / M1 ** 0.5), 0.2 * rn(C))
    h = rn(B, nv + N, W) * 1.3 + 0.2
    nodes = torch.tensor(real) if real is not None else torch.randint(1, N + 1, (B,), generator=g)
    mask = torch.cat([torch.ones(B, nv, dtype=torch.bool), torch.arange(N)[None, :] < nodes[:, None]], dim=1)
    target = rn(B, C) if loss == "mae" else torch.randint(0, C, (B,), generator=g)
    gr = gen("graph_head", cid, recipe)
    if recipe == "offset32":
        h = h + 32.0
    elif recipe == "const_rows":
        from conditioning import const_rows
        h, _ = const_rows(h, gr)
    elif recipe == "outliers":                                           # 1 % of the elements * 1000
        h = torch.where(torch.rand(h.shape, generator=gr) < 0.01, h * 1000.0, h)
    else:
        assert recipe == "plain", recipe
    return dict(id=cid, recipe=recipe, h=h, mask=mask, target=target, params=params, loss=loss, nv=nv, act=act, ln=ln,
                W=W, M0=M0, M1=M1, C=C, B=B, N=N)


def ref_head(h, target, mask, params, loss, nv, act):
    """(stats [3], y [B,C]) in the dtype of h, from the oracle's functions"""
    gamma, beta, W0, b0, W1, b1, Wt, bt = params
    x = h if gamma is None else O.layer_norm(h, gamma, beta)
    pooled = x[:, :nv].reshape(x.shape[0], nv * x.shape[2]) if nv else MO.masked_global_avg_pool_1d(x, mask)
    x = MO.mlp_out(pooled, {"mlp_out_0.kernel": W0, "mlp_out_0.bias": b0, "mlp_out_1.kernel": W1, "mlp_out_1.bias": b1}, 2, act)
    y = O.dense(x, Wt, bt)
    B, C = y.shape
    zero = torch.zeros((), dtype=y.dtype)
    if loss == "mae":
        return torch.stack([MO.mae_loss(y, target.to(y.dtype)) * (B * C), zero, zero + B * C]), y
    hits = (y.detach().argmax(-1) == target).to(y.dtype).sum()
    return torch.stack([MO.sparse_xent_loss(y, target) * B, hits, zero + B]), y


_REF = {}


def reference(cid, recipe="plain"):
    """(case, fp64 result): computed once, shared, never modified"""
    key = (cid, recipe)
    if key not in _REF:
        c = make_case(cid, recipe)
        h64 = c["h"].double().requires_grad_()
        p64 = tuple(None if p is None else p.double().requires_grad_() for p in c["params"])
        st, y = ref_head(h64, c["target"], c["mask"], p64, c["loss"], c["nv"], c["act"])
        gr = torch.autograd.grad(st[0] * S_UP, [h64] + [p for p in p64 if p is not None])
        y = y.detach()
        if c["loss"] == "mae":
            fair = float((y - c["target"].double()).abs().min())           # distance of |y - t| from its kink
        else:
            top = y.topk(2, dim=-1).values if y.shape[1] > 1 else torch.stack([y[:, 0] + 1, y[:, 0]], -1)
            fair = float((top[:, 0] - top[:, 1]).min())                     # gap between the two largest logits
        _REF[key] = (c, dict(stats=st.detach(), pred=y, d_h=gr[0], grads=list(gr[1:]), fair=fair))
    return _REF[key]


def run(fn, c, dev=None, up=S_UP, h=None):
    """fn = graph_head_loss / graph_head_composed on the case -> dict(stats, pred, d_h, grads) and the stats tensor"""
    mv = (lambda t: t.to(dev)) if dev is not None else (lambda t: t.clone())
    hh = mv(c["h"] if h is None else h).requires_grad_()
    ps = tuple(None if p is None else mv(p).requires_grad_() for p in c["params"])
    st, pred = fn(hh, mv(c["target"]), mv(c["mask"]), ps, c["loss"], c["nv"], c["act"])
    (st[0] * up).backward()
    return dict(stats=st.detach(), pred=pred.detach(), d_h=hh.grad, grads=[p.grad for p in ps if p is not None]), st


def grad_names(c):
    return NAMES if c["ln"] else NAMES[2:]


def zero_rows(c):
    """[B,nv+N] bool: the rows whose d_h is exactly zero by contract"""
    if c["nv"]:
        z = torch.ones_like(c["mask"])
        z[:, :c["nv"]] = False
        return z
    return ~c["mask"]
