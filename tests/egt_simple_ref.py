"""EGT-Simple ('bias' edge channels) composed from the oracle's primitives.

The model oracle's *_forward functions hard-code the residual layer loop; EGT-Simple (graph_xformer_model_base.py:173-190)
computes the edge tensor once in the embedding and never updates it: every layer projects gates and the logit bias from the
RAW e (no norm_edge), there is no dense_edge_r, no edge FFN (:313) and no edge_norm_final (:346).  This helper writes that
loop with O.block_forward(edge_channel_type="bias"), O.ffn_forward on the node channels, and the embedding / pooling /
mlp_out functions of oracle/egt_model_oracle.py.  tests/golden/model_egt_simple_small.npz (make_egt_simple_golden.py beside
it) pins it against drift."""
import os

import numpy as np
import torch

from oracle import egt_model_oracle as MO, egt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_egt_simple_small.npz")
BLOCK_KEYS = ("attention_gates.kernel", "attention_gates.bias", "dense_edge_b.kernel", "dense_edge_b.bias", "norm_mha.gamma",
              "norm_mha.beta", "dense_qkv.kernel", "dense_qkv.bias", "dense_mha.kernel", "dense_mha.bias")
FFN_KEYS = ("norm_gamma", "norm_beta", "lr1_kernel", "lr1_bias", "lr2_kernel", "lr2_bias")


def init_params(kind, cfg, generator):
    """MO.init_zinc_params restricted to the parameters an EGT-Simple model of `kind` ('zinc' | 'pattern' | 'cifar10') owns."""
    c = dict(cfg)
    if kind == "cifar10":
        c.setdefault("float_node_features", 5); c.setdefault("float_edge_features", 1)
    p = MO.init_zinc_params(c, dtype=torch.float32, generator=generator)
    gated = cfg.get("gate_attention", True)

    def keep(k):
        if k.startswith("edge_norm_final.") or ".ffn_edge." in k or ".norm_edge." in k or ".dense_edge_r." in k:
            return False
        if not gated and ".attention_gates." in k:
            return False
        if kind != "zinc" and k == "fm_emb.embeddings":
            return False
        if kind == "cifar10" and k == "node_emb.embeddings":
            return False
        return True
    return {k: v for k, v in p.items() if keep(k)}


def embeddings(kind, inp, p, cfg):
    dt = p["adj_emb.kernel"].dtype
    hops = MO.stack_hops(inp["graph_matrix"].to(dt), cfg["upto_hop"], cfg.get("clip_hops", True))
    e = O.dense(hops, p["adj_emb.kernel"], p["adj_emb.bias"])
    if kind == "cifar10":
        xn, mask = MO.keras_masking(inp["node_features"].to(dt), -1.0)
        h = O.dense(xn, p["node_emb.kernel"], p["node_emb.bias"])
        xe, _ = MO.keras_masking(inp["feature_matrix"].to(dt), -1.0)
        e = e + O.dense(xe, p["edge_emb.kernel"], p["edge_emb.bias"])
    else:
        h = MO.neg1_masked_embedding(inp["node_features"], p["node_emb.embeddings"])
        mask = O.node_mask_from_features(inp["node_features"])
        if kind == "zinc":
            e = e + MO.neg1_masked_embedding(inp["feature_matrix"], p["fm_emb.embeddings"])
    return h, e, mask


def forward(kind, inp, p, cfg, rand_masks=None):
    """-> (prediction, node mask).  zinc / cifar10: [B, num_targets] after the masked mean pool; pattern: per-node logits."""
    H, Ly, act = cfg.get("num_heads", 8), cfg["model_height"], cfg.get("activation", "elu")
    h, e, mask = embeddings(kind, inp, p, cfg)
    for ii in range(Ly):
        bp = {k: p[f"layer{ii}.{k}"] for k in BLOCK_KEYS if f"layer{ii}.{k}" in p}
        rm = None if rand_masks is None else rand_masks[ii]
        h, e_same = O.block_forward(h, e, mask, bp, num_heads=H, rand_mask=rm, edge_channel_type="bias",
                                    gate_attention=cfg.get("gate_attention", True))
        assert e_same is e                                                   # :190 returns e0
        h = O.ffn_forward(h, {k: p[f"layer{ii}.ffn_node.{k}"] for k in FFN_KEYS}, activation=act)   # :322-323, node channels only
    if cfg.get("do_final_norm", True):
        h = O.layer_norm(h, p["node_norm_final.gamma"], p["node_norm_final.beta"])
    x = h if kind == "pattern" else MO.masked_global_avg_pool_1d(h, mask)
    x = MO.mlp_out(x, p, len(cfg.get("mlp_layers", [0.5, 0.25])), act)
    return O.dense(x, p["target.kernel"], p["target.bias"]), mask


def small_case():
    """the committed golden's case: a ZINC-shaped EGT-Simple model, B = 3, N = 11, widths 32 / 8, two layers"""
    cfg = dict(model_width=32, edge_width=8, model_height=2, upto_hop=4, num_node_features=28, num_edge_features=4, num_targets=1)
    g = torch.Generator().manual_seed(20)
    B, N = 3, 11
    n = torch.tensor([11, 6, 9])
    real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
    adj = (torch.rand(B, N, N, generator=g) > 0.6).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
    tgt = torch.randn(B, 1, generator=g)
    params = init_params("zinc", cfg, g)
    return cfg, dict(node_features=nf, feature_matrix=fm, graph_matrix=adj, target=tgt), params


def small_case_outputs():
    cfg, inp, params = small_case()
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    y, _ = forward("zinc", inp, p64, cfg)
    loss = MO.mae_loss(y, inp["target"].double())
    gr = torch.autograd.grad(loss, list(p64.values()), allow_unused=True)
    out = {"y": y.detach().numpy(), "loss": loss.detach().numpy().reshape(1)}
    for k, g_ in zip(p64, gr):
        out["d/" + k] = np.zeros(tuple(p64[k].shape)) if g_ is None else g_.numpy()
    return out
