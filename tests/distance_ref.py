"""fp64 restatement of the distance objective (the reference's *_spe_do configs) and the inputs its tests share.

    target   lib/models/graph_model_base.py:66-76       hop_1 = A, hop_k = clip(A @ hop_{k-1}, 0, 1), round(sum of the first T)
    head     graph_model_base.py:83-94, graph_xformer_model_base.py:343-372
    loss     lib/base/genutil/loss_layers.py:38-67      sparse CE * (target > 0), summed per graph
"""
import math

import torch

HEAD_NAMES = ("edge_norm_final/gamma", "edge_norm_final/beta", "mlp_out_dist_targ_0/kernel", "mlp_out_dist_targ_0/bias",
              "mlp_out_dist_targ_1/kernel", "mlp_out_dist_targ_1/bias", "distance_target/kernel", "distance_target/bias")


def ref_target(adj, T):
    """graph_model_base.py:66-76; the clip is unconditional"""
    a = adj.double()
    hop, tot = a, a.clone()
    for _ in range(1, T):
        hop = torch.clamp(a @ hop, 0.0, 1.0)
        tot = tot + hop
    return torch.round(tot).to(torch.int64)


def ref_mlp_loss(ef, target, W0, b0, W1, b1, Wt, bt, activation):
    """the head behind edge_norm_final and the loss: per_graph [B]"""
    act = torch.nn.functional.elu if activation == "elu" else torch.relu
    x = act(ef @ W0 + b0)
    x = act(x @ W1 + b1)
    logits = x @ Wt + bt
    lse = torch.logsumexp(logits, dim=-1)
    ce = lse - logits.gather(-1, target[..., None])[..., 0]          # sparse categorical cross-entropy from logits
    return (ce * (target > 0).to(ce.dtype)).sum(dim=(1, 2))          # reduction 'sum' over the pairs of a graph


def ref_layer_norm(e, gamma, beta, eps=1e-3):
    mu = e.mean(dim=-1, keepdim=True)
    var = ((e - mu) ** 2).mean(dim=-1, keepdim=True)
    return (e - mu) / torch.sqrt(var + eps) * gamma + beta


def ref_head(e, target, params, activation="elu", eps=1e-3):
    """params: (gamma, beta, W0, b0, W1, b1, Wt, bt) fp64; gamma None = no edge_norm_final"""
    gamma, beta, *rest = params
    ef = e if gamma is None else ref_layer_norm(e, gamma, beta, eps)
    return ref_mlp_loss(ef, target, *rest, activation)


def lollipop(n_nodes, N):
    """triangle 0-1-2 plus the tail 2-3-...-(n_nodes-1); nodes n_nodes..N-1 isolated"""
    a = torch.zeros(N, N)
    edges = [(0, 1), (1, 2), (0, 2)] + [(i, i + 1) for i in range(2, n_nodes - 1)]
    for i, j in edges:
        a[i, j] = a[j, i] = 1.0
    return a


def make_graphs(N=19):
    """[3,N,N]: a 16-node lollipop, a 12-node one, and a graph with no edges at all"""
    return torch.stack([lollipop(min(16, N), N), lollipop(12, N), torch.zeros(N, N)])


def head_params(De, width, T, layernorm=True, seed=0):
    """fp32 head parameters (Keras shapes), all of them away from their initial values"""
    g = torch.Generator().manual_seed(1000 + seed)
    m0, m1, C = round(.5 * width), round(.25 * width), T + 1

    def glorot(fi, fo):
        lim = math.sqrt(6.0 / (fi + fo))
        return (torch.rand(fi, fo, generator=g) * 2 - 1) * lim

    vec = lambda n, base: base + 0.2 * torch.randn(n, generator=g)
    gamma, beta = (vec(De, 1.0), vec(De, 0.0)) if layernorm else (None, None)
    return (gamma, beta, glorot(De, m0), vec(m0, 0.0), glorot(m0, m1), vec(m1, 0.0), glorot(m1, C), vec(C, 0.0))


def tile_census(target_b):
    """(all-zero 16-pair tiles, mixed tiles) of one graph's flattened target"""
    t = target_b.reshape(-1)
    zero = mixed = 0
    for s in range(0, t.numel(), 16):
        c = t[s:s + 16]
        nz = int((c > 0).sum())
        zero += nz == 0
        mixed += 0 < nz < c.numel()
    return zero, mixed
