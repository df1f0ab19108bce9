"""fp64 restatement of the reference's virtual nodes -- TEST INFRASTRUCTURE, composed from oracle/egt_oracle.py and
oracle/egt_model_oracle.py the way tests/test_model.py composes them.  It follows the reference literally, with `cat`s:

    virtual_node_embedding   VirtualNodeEmbedding.call   lib/base/graph_layers/virtual_nodes.py:41-45
    virtual_edge_embedding   VirtualEdgeEmbedding.call   :86-99
    get_virtual_nodes        GetVirtualNodes.call        :130-133
    forward                  VNModel (lib/models/graph_model_base.py:212-268) around DCSVDTransformer of zinc/dc.py and
                             cifar10/dc.py: readout GetVirtualNodes -> Flatten -> mlp_out (zinc/dc.py:105-110)
"""
import math

import torch

from oracle import egt_model_oracle as MO, egt_oracle as O

VN_NODE = "virtual_node_embedding.virtual_node_embeddings"
VN_EDGE = "virtual_edge_embedding.virtual_edge_embeddings"


def virtual_node_embedding(h, emb):
    tiled = emb[None].repeat(h.shape[0], 1, 1)                        # tf.tile(expand_dims(embeddings, 0), [B, 1, 1])
    return torch.cat([tiled, h], dim=1)


def virtual_edge_embedding(e, emb):
    B, n1, n2, _ = e.shape
    emb_r, emb_c = emb[None, :, None, :], emb[None, None, :, :]
    tiled_row = emb_r.repeat(B, 1, n2, 1)
    tiled_col = emb_c.repeat(B, n1, 1, 1)
    tiled_box = (0.5 * (emb_r + emb_c)).repeat(B, 1, 1, 1)
    out = torch.cat([tiled_row, e], dim=1)
    bc = torch.cat([tiled_box, tiled_col], dim=1)
    return torch.cat([bc, out], dim=2)


def get_virtual_nodes(h, nv):
    return h[:, :nv, :]


def bordered_by_index(e, emb):
    """the same tensor from the index formulas (no cat): what the kernel's threads compute"""
    B, N, _, De = e.shape
    nv = emb.shape[0]
    out = torch.empty(B, nv + N, nv + N, De, dtype=e.dtype)
    for r in range(nv + N):
        for c in range(nv + N):
            if r >= nv and c >= nv:
                out[:, r, c] = e[:, r - nv, c - nv]
            elif r < nv and c < nv:
                out[:, r, c] = 0.5 * (emb[r] + emb[c])
            else:
                out[:, r, c] = emb[r] if r < nv else emb[c]
    return out


def embed_ref(fm, adj, table, W, b, vn, upto_hop, float_features=None, We=None, be=None):
    """the bordered edge embedding of egt_edge_embed_vn_fwd's inputs, in the dtype of the parameters"""
    e = O.dense(MO.stack_hops(adj.to(W.dtype), upto_hop), W, b) + MO.neg1_masked_embedding(fm, table)
    if float_features is not None:
        xe, _ = MO.keras_masking(float_features.to(W.dtype), -1.0)
        e = e + O.dense(xe, We, be)
    return virtual_edge_embedding(e, vn)


def init_params(kind, cfg, nv, generator):
    """MO.init_zinc_params plus the two virtual tables (O(1) values, like its randomised embeddings) and the first mlp_out
    kernel on the flattened virtual nodes [nv Dh, round(.5 Dh)]"""
    c = dict(cfg)
    if kind == "cifar10":
        c.update(float_node_features=5, float_edge_features=1)
    p = MO.init_zinc_params(c, dtype=torch.float64, generator=generator)
    if kind == "cifar10":
        p.pop("node_emb.embeddings"); p.pop("fm_emb.embeddings")
    Dh, De = cfg["model_width"], cfg["edge_width"]
    wo = p["mlp_out_0.kernel"].shape[1]
    lim = math.sqrt(6.0 / (nv * Dh + wo))
    p["mlp_out_0.kernel"] = (torch.rand(nv * Dh, wo, generator=generator, dtype=torch.float64) * 2 - 1) * lim
    p[VN_NODE] = torch.rand(nv, Dh, generator=generator, dtype=torch.float64) * 2 - 1
    p[VN_EDGE] = torch.rand(nv, De, generator=generator, dtype=torch.float64) * 2 - 1
    return {k: v.float() for k, v in p.items()}


def forward(kind, inp, p, cfg, nv):
    """prediction [B, num_targets] of the model with nv virtual nodes; kind 'zinc' | 'cifar10'; p in the compute dtype"""
    H, Ly = cfg.get("num_heads", 8), cfg["model_height"]
    act, ect = cfg.get("activation", "elu"), cfg.get("edge_channel_type", "residual")
    adj = inp["graph_matrix"]
    if kind == "zinc":
        h, e, _ = MO.zinc_embeddings(inp["node_features"], inp["feature_matrix"], adj, p, cfg)
        mask = O.node_mask_from_features(inp["node_features"], nv)
    else:
        dt = p["node_emb.kernel"].dtype
        xn, _ = MO.keras_masking(inp["node_features"].to(dt), -1.0)
        h = O.dense(xn, p["node_emb.kernel"], p["node_emb.bias"])
        xe, _ = MO.keras_masking(inp["feature_matrix"].to(dt), -1.0)
        e = O.dense(xe, p["edge_emb.kernel"], p["edge_emb.bias"])
        e = e + O.dense(MO.stack_hops(adj.to(dt), cfg["upto_hop"], cfg.get("clip_hops", True)), p["adj_emb.kernel"], p["adj_emb.bias"])
        mask = O.node_mask_from_masking(inp["node_features"], -1.0, nv)
    h = virtual_node_embedding(h, p[VN_NODE])                         # VNModel.combine_node_embeddings
    e = virtual_edge_embedding(e, p[VN_EDGE])                         # VNModel.combine_edge_embeddings
    M = O.constrained_edge_mask(adj.to(h.dtype), H, nv) if ect == "constrained" else None   # VNModel.get_edge_mask
    for ii in range(Ly):
        bp = {k[len(f"layer{ii}."):]: v for k, v in p.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
        h, e = O.block_forward(h, e, mask, bp, num_heads=H, attn_mask=M, edge_channel_type=ect)
        if ect != "bias":
            e = O.ffn_forward(e, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_edge.")}, activation=act)
        h = O.ffn_forward(h, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_node.")}, activation=act)
    h = O.layer_norm(h, p["node_norm_final.gamma"], p["node_norm_final.beta"])
    x = get_virtual_nodes(h, nv).reshape(h.shape[0], nv * h.shape[2])  # GetVirtualNodes -> Flatten
    x = MO.mlp_out(x, p, len(cfg.get("mlp_layers", [0.5, 0.25])), act)
    return O.dense(x, p["target.kernel"], p["target.bias"])


def module_param(model, key):
    """oracle parameter name -> the model's parameter (None: the model has no such parameter)"""
    if key == VN_NODE:
        return model.virtual_node_emb
    if key == VN_EDGE:
        return model.virtual_edge_emb
    if key in ("node_emb.embeddings", "fm_emb.embeddings"):
        t = getattr(model, key.split(".")[0])
        return t if isinstance(t, torch.nn.Parameter) else None
    parts = key.split(".")
    try:
        if parts[0].startswith("layer"):
            ii = int(parts[0][5:])
            if parts[1].startswith("ffn_"):
                lst = model.layers.ffn_node if parts[1] == "ffn_node" else model.layers.ffn_edge
                return None if lst is None else getattr(lst[ii], parts[2])
            return getattr(getattr(model.layers.blocks[ii], parts[1]), parts[2])
        if parts[0].startswith("mlp_out_"):
            return getattr(model.mlp_out[int(parts[0][8:])], parts[1])
        return getattr(getattr(model, parts[0]), parts[1])
    except AttributeError:
        return None


def graphs(kind, B, N, counts, generator):
    """a padded batch: node counts `counts` (padded to N), symmetric 0/1 adjacency without self loops among the real nodes"""
    g = generator
    real = torch.arange(N)[None, :] < torch.tensor(counts)[:, None]
    adj = (torch.rand(B, N, N, generator=g) > 0.6).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    inp = dict(graph_matrix=adj)
    if kind == "cifar10":
        nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
        fm = torch.where(adj > 0, torch.rand(B, N, N, generator=g), torch.tensor(-1.0))[..., None]
        inp.update(node_features=nf, feature_matrix=fm, target=torch.randint(0, 10, (B,), generator=g))
    else:
        nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
        fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
        inp.update(node_features=nf, feature_matrix=fm, target=torch.randn(B, 1, generator=g))
    return inp
