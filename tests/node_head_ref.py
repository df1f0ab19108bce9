"""fp64 restatement of the node-classification readout and its loss (PATTERN / CLUSTER) and the inputs its tests share.

    head   lib/models/sbm_pattern/dc.py:51-58, graph_xformer_model_base.py:343-372   node_norm_final -> mlp_out -> Dense(C)
    loss   lib/base/genutil/losses.py:41-118     class-weighted sparse cross-entropy; the node mask as sample weight
    stats  = [sum mask w[y] CE(z, y),  sum mask [argmax z == y],  sum mask]
"""
import math

import torch

NAMES = ("node_norm_final/gamma", "node_norm_final/beta", "mlp_out_0/kernel", "mlp_out_0/bias", "mlp_out_1/kernel",
         "mlp_out_1/bias", "target/kernel", "target/bias")


def ref_layer_norm(x, gamma, beta, eps=1e-3):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def ref_logits(h, params, activation="elu", eps=1e-3):
    """params: (gamma, beta, W0, b0, W1, b1, Wt, bt); gamma None = no node_norm_final"""
    gamma, beta, W0, b0, W1, b1, Wt, bt = params
    act = torch.nn.functional.elu if activation == "elu" else torch.relu
    x = h if gamma is None else ref_layer_norm(h, gamma, beta, eps)
    x = act(x @ W0 + b0)
    x = act(x @ W1 + b1)
    return x @ Wt + bt


def ref_stats(h, target, mask, class_weights, params, activation="elu", eps=1e-3):
    """-> (stats [3], logits [B,N,C]); a masked slot's target is replaced before it is used as an index"""
    z = ref_logits(h, params, activation, eps)
    m = mask.to(z.dtype)
    y = torch.where(mask, target, torch.zeros_like(target)).long()
    ce = torch.logsumexp(z, dim=-1) - z.gather(-1, y[..., None])[..., 0]
    loss = (class_weights.to(z.dtype)[y] * ce * m).sum()
    hit = ((z.argmax(-1) == y) & mask).sum().to(z.dtype)       # torch.argmax: the lowest index on a tie
    return torch.stack([loss, hit, m.sum()]), z


def head_params(W, width, C, layernorm=True, seed=0):
    """fp32 head parameters (Keras shapes), all of them away from their initial values"""
    g = torch.Generator().manual_seed(2000 + seed)
    m0, m1 = round(.5 * width), round(.25 * width)

    def glorot(fi, fo):
        lim = math.sqrt(6.0 / (fi + fo))
        return (torch.rand(fi, fo, generator=g) * 2 - 1) * lim

    vec = lambda n, base: base + 0.2 * torch.randn(n, generator=g)
    gamma, beta = (vec(W, 1.0), vec(W, 0.0)) if layernorm else (None, None)
    return (gamma, beta, glorot(W, m0), vec(m0, 0.0), glorot(m0, m1), vec(m1, 0.0), glorot(m1, C), vec(C, 0.0))


LENGTHS = {(3, 19): (19, 0, 14), (2, 16): (16, 16), (4, 70): (70, 0, 33, 61)}     # real nodes per graph (0: masked entirely)


def make_inputs(B, N, W, C, seed=0):
    """h [B,N,W], target [B,N] int64, mask [B,N] bool, class_weights [C].  Unmasked targets cycle through every class; masked
    targets alternate between -1, a value >= C and 0 (none of them may have any effect)."""
    g = torch.Generator().manual_seed(31 + seed)
    n = torch.tensor(LENGTHS[(B, N)])
    mask = torch.arange(N)[None, :] < n[:, None]
    h = torch.randn(B, N, W, generator=g) * 1.5 + 0.3
    flat = torch.arange(B * N)
    perm = torch.randperm(C, generator=g)
    target = perm[flat % C].reshape(B, N).clone()
    junk = torch.tensor([-1, C + 3, 0])[flat % 3].reshape(B, N)
    target = torch.where(mask, target, junk)
    sizes = torch.arange(1, C + 1, dtype=torch.float32) * 100 + 17          # class weights as class_weights_from_sizes builds them
    cw = sizes.sum() - sizes
    return dict(h=h, target=target, mask=mask, class_weights=cw / cw.sum())


def tile_census(mask):
    """(tiles with 16 real rows, partly masked tiles, tiles without a real row, rows of the last tile) over the flattened rows"""
    m = mask.reshape(-1)
    full = part = none = 0
    for s in range(0, m.numel(), 16):
        c = m[s:s + 16]
        k = int(c.sum())
        full += k == 16
        none += k == 0
        part += 0 < k < c.numel()
    return full, part, none, m.numel() - 16 * ((m.numel() - 1) // 16)


def top2_gap(logits, mask):
    """smallest gap between the two largest logits over the unmasked rows"""
    t = logits.topk(2, dim=-1).values
    return float((t[..., 0] - t[..., 1])[mask].min())


def workgroups(B, N):
    """the library's chunking rule (egt_head.hip node_head_groups): a workgroup has four waves of one 16-row tile each, so at
    least four tiles per workgroup, at most 1024 workgroups -> (workgroups, tiles per workgroup)"""
    tiles = (B * N + 15) // 16
    G = max(1, min(1024, tiles // 4))
    return G, (tiles + G - 1) // G
