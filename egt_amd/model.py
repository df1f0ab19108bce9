"""The ZINC model around the attention path: what the reference's
``lib.models.zinc.dc.DCSVDTransformer`` builds for scheme ``zinc.svd`` with the shipped configs
(``use_svd: false``, ``configs/main/zinc/*/egt.json``), as one torch module

    ZincDCTransformer(**model_config)(node_features, feature_matrix, graph_matrix) -> [B, num_targets]

Pair-sized work runs in the HIP kernels through the C-ABI: the edge-channel input embedding
(egt_edge_embed_fwd/bwd: hop stacking + adj_emb + fm_emb), every attention block (egt_block_*) and
every channel FFN (egt_ffn_*), the node mask producer (egt_node_mask_from_features).  The node input
(embedding lookup or Masking + Dense, SVD / eigenvector encoding, virtual rows, node mask) is one fused op (`inputs` ->
egt_amd.node_embed: egt_node_embed_fwd/bwd), and so are the readout + loss of a training step (graph_loss -> egt_amd.graph_head,
classification_loss -> egt_amd.node_head); each has its composed torch route for CPU tensors and uncovered geometries.
num_virtual_nodes > 0 (ZINC / CIFAR10): the embedding kernel writes e with its border of
virtual edge embeddings (egt_edge_embed_vn_fwd/bwd), the node-input kernel puts the virtual node rows in front of h, the readout takes them.  Parameters carry the reference's Keras variable names (keras_named_parameters) so a
weight file of the reference loads unchanged.

Reference (relative to /root/reference/): lib/models/zinc/dc.py:17-120,
lib/models/graph_model_base.py:97-129, lib/models/graph_xformer_model_base.py:336-372,377-466,
lib/training/schemes/zinc/svd.py:27-42, lib/training/schemes/scheme_base.py:37-60.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
import torch.nn.functional as F

from . import _lib as L
from .functional import _f32c, _need_gpu
from .layers import EGTLayerStack, KerasDense, KerasLayerNorm, LN_EPS
from .masks import node_mask_from_features


# edge_dtype keyword of the models / edge_embed -> storage dtype of the edge tensor e (EGT_BF16: bf16 in HBM, fp32 math)
EDGE_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _edge_dtype(edge_dtype) -> torch.dtype:
    if edge_dtype not in EDGE_DTYPES:
        raise ValueError(f"edge_dtype must be one of {sorted(EDGE_DTYPES)} (got {edge_dtype!r})")
    return EDGE_DTYPES[edge_dtype]


def _embed_desc(B, N, De, upto_hop, clip_hops, num_edge_features, num_float_features=0, mask_value=-1.0,
                dtype=torch.float32) -> L.EmbedDesc:
    return L.EmbedDesc(B=B, N=N, De=De, upto_hop=upto_hop, clip_hops=1 if clip_hops else 0,
                       num_edge_features=num_edge_features, dtype=L.EGT_BF16 if dtype == torch.bfloat16 else L.EGT_F32,
                       num_float_features=num_float_features, mask_value=float(mask_value), reserved=0)


class _EdgeEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmat, adj, table, kernel, bias, clip_hops, ffeat=None, mask_value=-1.0, e_dtype=torch.float32, vn=None):
        """kernel: [upto_hop + F, De] (adj_emb rows, then the rows of the real-valued features' Dense); ffeat [B,N,N,F];
        e_dtype: storage of e (fp32 or bf16; the hop planes and every parameter gradient stay fp32); vn [nv,De]: the virtual
        edge table -- e comes out bordered, [B,nv+N,nv+N,De] (egt_edge_embed_vn_*)"""
        _need_gpu(fmat, adj, table)
        lib = L.load()
        fmat = fmat.to(torch.int32).contiguous()
        adj = _f32c(adj.to(torch.float32))
        table, kernel, bias = _f32c(table), _f32c(kernel), _f32c(bias)
        ffeat = None if ffeat is None else _f32c(ffeat.to(torch.float32))
        B, N, _ = adj.shape
        F_ = 0 if ffeat is None else ffeat.shape[-1]
        K, De = kernel.shape[0] - F_, kernel.shape[1]
        desc = _embed_desc(B, N, De, K, clip_hops, table.shape[0] - 1, F_, mask_value, e_dtype)
        if not lib.egt_edge_embed_supported(C.byref(desc)):
            raise ValueError(f"edge embedding kernel does not cover upto_hop={K}, edge_width={De}, "
                             f"num_edge_features={table.shape[0] - 1}")
        hops = torch.empty(K + F_, B, N, N, dtype=torch.float32, device=adj.device)   # plane-major (unit-stride planes)
        nv = 0 if vn is None else int(vn.shape[0])
        if vn is None:
            e = torch.empty(B, N, N, De, dtype=e_dtype, device=adj.device)
            L.check(lib.egt_edge_embed_fwd(C.byref(desc), L.ptr(fmat), L.ptr(adj), L.ptr(ffeat), L.ptr(table), L.ptr(kernel),
                                           L.ptr(bias), L.ptr(hops), L.ptr(e), L.current_stream()))
        else:
            vn = _f32c(vn)
            if vn.dim() != 2 or vn.shape[1] != De or not lib.egt_edge_embed_vn_supported(C.byref(desc), nv):
                raise ValueError(f"bordered edge embedding kernel does not cover a virtual edge table {tuple(vn.shape)} "
                                 f"(1..16 rows of edge_width={De})")
            e = torch.empty(B, nv + N, nv + N, De, dtype=e_dtype, device=adj.device)
            L.check(lib.egt_edge_embed_vn_fwd(C.byref(desc), nv, L.ptr(fmat), L.ptr(adj), L.ptr(ffeat), L.ptr(table),
                                              L.ptr(kernel), L.ptr(bias), L.ptr(vn), L.ptr(hops), L.ptr(e), L.current_stream()))
        ctx.desc, ctx.nv = desc, nv
        ctx.save_for_backward(fmat, hops, table, kernel, bias)
        ctx.mark_non_differentiable(hops)
        return e, hops

    @staticmethod
    def backward(ctx, de, _dhops):
        lib = L.load()
        fmat, hops, table, kernel, bias = ctx.saved_tensors
        desc = ctx.desc
        de = de.to(torch.bfloat16 if desc.dtype == L.EGT_BF16 else torch.float32).contiguous()
        dt, dk, db = torch.empty_like(table), torch.empty_like(kernel), torch.empty_like(bias)
        if ctx.nv:
            dvn = torch.empty(ctx.nv, desc.De, dtype=torch.float32, device=de.device)
            ws = torch.empty(lib.egt_edge_embed_vn_workspace_bytes(C.byref(desc), ctx.nv), dtype=torch.uint8, device=de.device)
            L.check(lib.egt_edge_embed_vn_bwd(C.byref(desc), ctx.nv, L.ptr(fmat), L.ptr(hops), L.ptr(de), L.ptr(dt), L.ptr(dk),
                                              L.ptr(db), L.ptr(dvn), L.ptr(ws), L.current_stream()))
            return None, None, dt, dk, db, None, None, None, None, dvn
        ws = torch.empty(lib.egt_edge_embed_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=de.device)
        L.check(lib.egt_edge_embed_bwd(C.byref(desc), L.ptr(fmat), L.ptr(hops), L.ptr(de), L.ptr(dt), L.ptr(dk),
                                       L.ptr(db), L.ptr(ws), L.current_stream()))
        return None, None, dt, dk, db, None, None, None, None, None


def edge_embed(feature_matrix, graph_matrix, fm_table, adj_kernel, adj_bias, clip_hops=True, return_hops=False,
               float_features=None, float_kernel=None, float_bias=None, mask_value=-1.0, edge_dtype="f32",
               virtual_edge_table=None):
    """e0 = fm_table[feature_matrix + 1] + stack_hops(graph_matrix) @ adj_kernel + adj_bias
          [+ Dense(Masking(float_features))]  ->  [B,N,N,De].
    float_features [B,N,N,F] (F <= 4) with its Dense kernel [F,De] / bias: the real-valued edge features of the
    CIFAR10 / MNIST models (lib/models/cifar10/dc.py:70-73); they ride as F more planes behind the hop planes.
    edge_dtype "bf16": e is stored in bfloat16 (the fp32 sum rounded once, to nearest even); its gradient flows back
    in bf16 and the parameter gradients stay fp32.
    virtual_edge_table [nv,De] (1 <= nv <= 16): e0 bordered with the virtual nodes' edge embeddings as rows, columns and the
    corner box 0.5 (vn[i] + vn[j]) (VirtualEdgeEmbedding, virtual_nodes.py:86-99) -> [B,nv+N,nv+N,De], written by one kernel;
    the table's gradient is fp32."""
    kernel, bias = adj_kernel, adj_bias
    if float_features is not None:
        kernel = torch.cat([adj_kernel, float_kernel], dim=0)        # autograd splits the gradient rows back
        bias = adj_bias + float_bias
    e, hops = _EdgeEmbed.apply(feature_matrix, graph_matrix, fm_table, kernel, bias, clip_hops, float_features, mask_value,
                               _edge_dtype(edge_dtype), virtual_edge_table)
    return (e, hops) if return_hops else e


class ZincDCTransformer(nn.Module):
    """DCSVDTransformer for zinc.svd without SVD features; constructor kwargs are the reference's
    model_config keys (scheme_base.py:37-60, zinc/svd.py:27-35) with its defaults."""
    HAS_VIRTUAL_NODES = True      # the reference class derives from VNModel (zinc/dc.py, cifar10/dc.py)

    def __init__(self, model_width=64, edge_width=64, num_heads=8, model_height=10, gate_attention=True,
                 edge_channel_type='residual', upto_hop=16, clip_hops=True, random_mask_prob=0.1,
                 clip_logits_value=[-5, 5], mlp_layers=[.5, .25], activation='elu', do_final_norm=True,
                 ffn_multiplier=2., num_node_features=28, num_edge_features=4, num_targets=1,
                 readout_edges=False, num_virtual_nodes=0, node_dropout=0., edge_dropout=0.,
                 # positional encodings (SVDFeatModel / EigFeatModel, graph_model_base.py:284-414)
                 use_svd=False, num_svd_features=256, sel_svd_features=128, random_neg=False, transform_svd=False,
                 use_eig=False, num_eig_features=40, sel_eig_features=20, transform_eig=False,
                 # operator attributes handed to every attention block (graph_xformer_model_base.py:117-127)
                 scale_degree=False, scaler_type='log', attn_dropout=0., edge_activation=None,
                 # reference keys that are accepted at their default only (each would change the model: no silent ignore)
                 l2_reg=0, distance_loss=0., distance_target=8, add_n_norm=False, combine_layer_repr=False,
                 node2edge_xtalk=0., edge2node_xtalk=0., node2edge_embed=False, node_normalization='layer',
                 edge_normalization='layer', global_step_layer=False, max_length=None,
                 seed=0, ffn_matmul='f32', edge_dtype='f32', fused_attn_dropout=False, **unknown):
        super().__init__()
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown model_config keys {sorted(unknown)}")
        # fused_attn_dropout (a project key): attn_dropout > 0 drawn inside the fused pair kernels (EGTBlock) instead of sending
        # every layer to the composed operator; off by default
        if not isinstance(fused_attn_dropout, bool):
            raise ValueError(f"fused_attn_dropout must be True or False (got {fused_attn_dropout!r})")
        self.fused_attn_dropout = fused_attn_dropout
        # edge_dtype (a project key, like ffn_matmul): storage of the [B,N,N,De] edge tensor between the edge embedding, the
        # attention blocks and the edge FFNs.  "bf16" halves its HBM traffic; node tensors, parameters and math stay fp32.
        self.edge_dtype = _edge_dtype(edge_dtype)
        unsupported = dict(readout_edges=(readout_edges, False),
                           node_dropout=(node_dropout, 0), edge_dropout=(edge_dropout, 0), l2_reg=(l2_reg, 0),
                           add_n_norm=(add_n_norm, False),
                           combine_layer_repr=(combine_layer_repr, False), node2edge_embed=(node2edge_embed, False),
                           node_normalization=(node_normalization, 'layer'), edge_normalization=(edge_normalization, 'layer'))
        bad = {k: v for k, (v, d) in unsupported.items() if v != d}
        if bad:    # the reference model applies every one of these: training "a different model without a warning" is not an option
            raise NotImplementedError(f"{type(self).__name__} covers the shipped configs; not built: {bad}")
        # cross-talk in the FFN (egt_amd.xtalk): fp32 edge tensors, no virtual nodes; with 'bias' edge channels there is no edge
        # FFN, the reference never runs the exchange and the model is the one without the keys
        for k, v in (("node2edge_xtalk", node2edge_xtalk), ("edge2node_xtalk", edge2node_xtalk)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not 0 <= v <= 1:
                raise ValueError(f"{k} must be a fraction in [0, 1] (got {v!r})")
        if node2edge_xtalk > 0 or edge2node_xtalk > 0:
            why = {}
            if self.edge_dtype != torch.float32:
                why["edge_dtype"] = edge_dtype
            if int(num_virtual_nodes):
                why["num_virtual_nodes"] = num_virtual_nodes
            if edge_channel_type not in ('residual', 'constrained', 'bias'):
                why["edge_channel_type"] = edge_channel_type
            if why:
                raise NotImplementedError(f"{type(self).__name__} covers the shipped configs; not built: node2edge_xtalk="
                                          f"{node2edge_xtalk}, edge2node_xtalk={edge2node_xtalk} with {why}")
        # virtual nodes (VNModel, graph_model_base.py:212-281): nv learned node embeddings in front of h, e bordered with nv
        # learned edge embeddings, the graph-level readout taken from the virtual nodes (zinc/dc.py:105-110)
        nv = self.num_virtual_nodes = int(num_virtual_nodes)
        if nv and not self.HAS_VIRTUAL_NODES:
            raise NotImplementedError(f"{type(self).__name__}: num_virtual_nodes={nv} (the reference model has no VNModel)")
        if nv < 0 or nv > 16:
            raise NotImplementedError(f"{type(self).__name__} covers the shipped configs; not built: num_virtual_nodes={nv} "
                                      f"(the bordered edge embedding takes 1..16)")
        if nv and float(distance_loss) > 0:   # the reference crops the border before the head; no shipped config combines them
            raise NotImplementedError(f"{type(self).__name__} covers the shipped configs; not built: distance_loss={distance_loss} "
                                      f"together with num_virtual_nodes={nv}")
        # distance objective (the *_spe_do configs): built for the head geometries of the shipped model widths (egt_amd/head.py)
        self.distance_loss = float(distance_loss)
        if self.distance_loss > 0:
            why = {}
            if edge_channel_type not in ('residual', 'constrained'):
                why["edge_channel_type"] = edge_channel_type
            if list(mlp_layers) != [.5, .25]:
                why["mlp_layers"] = list(mlp_layers)
            if model_width not in (48, 64):
                why["model_width"] = model_width
            if not (isinstance(distance_target, int) and 1 <= distance_target <= 15):
                why["distance_target"] = distance_target
            if why:
                raise NotImplementedError(f"{type(self).__name__} covers the shipped configs; not built: distance_loss="
                                          f"{distance_loss} with {why}")
        # 'bias' = EGT-Simple (configs/ablation/egt_simple): e is computed once by the embedding and never updated; no
        # norm_edge, dense_edge_r, edge FFN or edge_norm_final (graph_xformer_model_base.py:173-190, :313, :346).  Built for the
        # head dims the fused block covers (d <= 8): the ZINC egt_simple configs (model_width 80, d = 10) stay refused.
        if edge_channel_type not in ('residual', 'constrained', 'bias') or \
                (edge_channel_type == 'bias' and model_width > 8 * num_heads):
            raise NotImplementedError("edge_channel_type must be residual or constrained")
        if use_svd and use_eig:
            raise NotImplementedError("use_svd and use_eig together (no reference model class mixes both)")
        self.cfg = dict(model_width=model_width, edge_width=edge_width, num_heads=num_heads, model_height=model_height,
                        upto_hop=upto_hop, clip_hops=clip_hops, mlp_layers=list(mlp_layers), activation=activation,
                        do_final_norm=do_final_norm, num_node_features=num_node_features,
                        num_edge_features=num_edge_features, num_targets=num_targets, ffn_multiplier=ffn_multiplier,
                        edge_channel_type=edge_channel_type, distance_target=distance_target,
                        use_svd=bool(use_svd), num_svd_features=num_svd_features, sel_svd_features=sel_svd_features,
                        transform_svd=bool(transform_svd), use_eig=bool(use_eig), num_eig_features=num_eig_features,
                        sel_eig_features=sel_eig_features, transform_eig=bool(transform_eig), random_neg=bool(random_neg))
        self.node_emb = nn.Parameter(torch.empty(num_node_features + 1, model_width).uniform_(-0.05, 0.05))   # keras 'uniform'
        self.fm_emb = nn.Parameter(torch.empty(num_edge_features + 1, edge_width).uniform_(-0.05, 0.05))
        self.adj_emb = KerasDense(upto_hop, edge_width)
        if nv:                                                                           # virtual_nodes.py:31-37, :76-82
            self.virtual_node_emb = nn.Parameter(torch.empty(nv, model_width).uniform_(-0.05, 0.05))
            self.virtual_edge_emb = nn.Parameter(torch.empty(nv, edge_width).uniform_(-0.05, 0.05))
        if use_svd and transform_svd:
            self.svd_emb = KerasDense(2 * sel_svd_features, model_width)                # graph_model_base.py:343-345
        if use_eig and transform_eig:
            self.eig_emb = KerasDense(sel_eig_features, model_width)                    # :408-410
        self.layers = EGTLayerStack(model_height=model_height, model_width=model_width, edge_width=edge_width,
                                    activation=activation, num_heads=num_heads, gate_attention=gate_attention,
                                    edge_channel_type=edge_channel_type, clip_logits_value=clip_logits_value,
                                    random_mask_prob=random_mask_prob, scale_degree=scale_degree, scaler_type=scaler_type,
                                    attn_dropout=attn_dropout, edge_activation=edge_activation, seed=seed,
                                    fused_attn_dropout=fused_attn_dropout,
                                    # the operator reads num_virtual_nodes in its degree scaler only (egt_layers.py:123-136)
                                    num_virtual_nodes=nv if scale_degree else 0,
                                    ffn_matmul=ffn_matmul, ffn_multiplier=ffn_multiplier,
                                    node2edge_xtalk=node2edge_xtalk, edge2node_xtalk=edge2node_xtalk)
        if self.edge_dtype == torch.bfloat16:
            self.layers.check_edge_dtype(self.edge_dtype)   # ValueError now, not a TypeError at the first step
        self.node_norm_final = KerasLayerNorm(model_width) if do_final_norm else None
        self.mlp_out = nn.ModuleList()
        w = max(nv, 1) * model_width                  # GetVirtualNodes -> Flatten: [B, nv Dh] (zinc/dc.py:105-108)
        for f in mlp_layers:
            self.mlp_out.append(KerasDense(w, round(f * model_width)))
            w = round(f * model_width)
        self.target = KerasDense(w, num_targets)
        self.dist_head = None
        if self.distance_loss > 0:
            from .head import DistanceHead
            try:   # the library decides the coverage (egt_edge_head_supported), with the edge dtype the model runs in
                self.dist_head = DistanceHead(edge_width, model_width, distance_target, mlp_layers, activation, do_final_norm,
                                              self.edge_dtype)
            except NotImplementedError as ex:
                raise NotImplementedError(f"{type(self).__name__} covers the shipped configs; not built: distance_loss="
                                          f"{distance_loss} ({ex})") from None

    # ---- positional encodings: node_emb_add = Add()([node embedding, PE embedding]) (graph_xformer_model_base.py:390-399) ----
    def positional(self, h, singular_vectors=None, eigen_vectors=None, pe_signs=None):
        """h + the SVD / eigenvector embedding of the batch.  Training applies the reference's random sign flip
        (RandomNeg / RandomNegEig, misc.py:53-94): one sign per (graph, feature), drawn on the device unless `pe_signs`
        ([B,1,F,1] for SVD, [B,1,F] for eigenvectors) injects the sample."""
        from .node_embed import positional_composed
        c = self.cfg
        draw = bool(c["random_neg"] and self.training)
        signs = pe_signs if draw else None
        if c["use_svd"]:
            if singular_vectors is None:
                raise ValueError("use_svd=True: the batch must carry singular_vectors [B,N,num_svd_features,2]")
            h = positional_composed(h, singular_vectors, "svd", c["sel_svd_features"], c["transform_svd"], self._pe_dense(), signs, draw)
        if c["use_eig"]:
            if eigen_vectors is None:
                raise ValueError("use_eig=True: the batch must carry eigen_vectors [B,N,num_eig_features]")
            h = positional_composed(h, eigen_vectors, "eig", c["sel_eig_features"], c["transform_eig"], self._pe_dense(), signs, draw)
        return h

    def _pe_dense(self):
        """(kernel, bias) of svd_emb / eig_emb, None where the encoding is added without a Dense"""
        m = getattr(self, "svd_emb", None) or getattr(self, "eig_emb", None)
        return None if m is None else (m.kernel, m.bias)

    def edge_mask(self, graph_matrix, attn_mask):
        """'constrained' edge channels: M = the adjacency tiled over the heads (AdjMatModel.get_edge_mask,
        graph_model_base.py:131-142), ones to and from the virtual nodes (VNModel.get_edge_mask, :248-268), unless the
        caller passes its own."""
        if attn_mask is None and self.cfg["edge_channel_type"] == 'constrained':
            from .masks import constrained_edge_mask
            return constrained_edge_mask(graph_matrix, self.cfg["num_heads"], self.num_virtual_nodes)
        return attn_mask

    def with_virtual_nodes(self, h):
        """[B,N,Dh] -> [B,nv+N,Dh]: the virtual-node embeddings in front of every graph's nodes, AFTER the positional
        encodings were added to the real nodes (VNModel.combine_node_embeddings, graph_model_base.py:227-235)"""
        if not self.num_virtual_nodes:
            return h
        from .node_embed import virtual_rows_composed
        return virtual_rows_composed(h, self.virtual_node_emb)

    def graph_readout(self, h, mask):
        """[B,N',Dh] -> [B, .]: the virtual nodes' rows flattened (GetVirtualNodes -> Flatten, zinc/dc.py:105-108), or the
        masked mean over the nodes (node_glob_avg_pool, :109) in a model without virtual nodes"""
        nv = self.num_virtual_nodes
        if nv:
            return h[:, :nv].reshape(h.shape[0], nv * h.shape[2])
        m = mask.to(h.dtype)[..., None]
        return (h * m).sum(dim=1) / m.sum(dim=1)

    # the Keras functional model contains only layers on a path to the outputs: with readout_edges=False the last
    # layer's dense_edge_r / edge FFN and edge_norm_final are NOT part of the reference model
    def _dead_edge_params(self):
        if self.cfg["edge_channel_type"] == 'bias':
            return []                    # EGT-Simple: every layer's gate and bias projections feed h; nothing else is edge-side
        if self.dist_head is not None:
            return []                    # the distance objective reads the final edge channels: the whole edge side is live
        if self.layers.xtalk and self.layers.xtalk[1] > 0:
            f = self.layers.ffn_edge[-1]   # edge -> node cross-talk: the last fnn_lr1_edge feeds the nodes, only fnn_lr2_edge is dead
            return [f.lr2_kernel, f.lr2_bias]
        last = self.layers.blocks[-1]
        dead = [last.dense_edge_r.kernel, last.dense_edge_r.bias]
        if self.layers.ffn_edge is not None:
            dead += list(self.layers.ffn_edge[-1].parameters())
        return dead

    def keras_named_parameters(self):
        dead = {id(p) for p in self._dead_edge_params()}
        out = {"adj_emb/kernel": self.adj_emb.kernel, "adj_emb/bias": self.adj_emb.bias}
        if hasattr(self, "svd_emb"):
            out["svd_emb/kernel"], out["svd_emb/bias"] = self.svd_emb.kernel, self.svd_emb.bias
        if hasattr(self, "eig_emb"):
            out["eig_emb/kernel"], out["eig_emb/bias"] = self.eig_emb.kernel, self.eig_emb.bias
        if isinstance(self.node_emb, nn.Parameter):
            out["node_emb/embeddings"] = self.node_emb
        if isinstance(self.fm_emb, nn.Parameter):
            out["fm_emb/embeddings"] = self.fm_emb
        if self.num_virtual_nodes:
            out["virtual_node_embedding/virtual_node_embeddings"] = self.virtual_node_emb
            out["virtual_edge_embedding/virtual_edge_embeddings"] = self.virtual_edge_emb
        out.update({k: v for k, v in self.layers.keras_named_parameters().items() if id(v) not in dead})
        if self.node_norm_final is not None:
            out["node_norm_final/gamma"] = self.node_norm_final.gamma
            out["node_norm_final/beta"] = self.node_norm_final.beta
        for i, m in enumerate(self.mlp_out):
            out[f"mlp_out_{i}/kernel"], out[f"mlp_out_{i}/bias"] = m.kernel, m.bias
        out["target/kernel"], out["target/bias"] = self.target.kernel, self.target.bias
        if self.dist_head is not None:
            out.update(self.dist_head.keras_named_parameters())
        return out

    def trainable_parameters(self):
        """the parameters the reference model owns (the dead last-layer edge parameters excluded)"""
        return list(self.keras_named_parameters().values())

    def _edge_key(self):
        return "bf16" if self.edge_dtype == torch.bfloat16 else "f32"

    def _virtual_edge_table(self):
        return self.virtual_edge_emb if self.num_virtual_nodes else None

    def _node_embedding(self, node_features):
        """h [B,N,Dh] of the real nodes and the mask [B,nv+N] from the composed ops"""
        mask = node_mask_from_features(node_features, self.num_virtual_nodes)           # masking.py:42-43, virtual_nodes.py:47-50
        h = F.embedding((node_features + 1).long(), self.node_emb)                      # zinc/dc.py:66-69
        return h, mask

    def _edge_embedding(self, feature_matrix, graph_matrix):
        return edge_embed(feature_matrix, graph_matrix, self.fm_emb, self.adj_emb.kernel, self.adj_emb.bias,
                          clip_hops=self.cfg["clip_hops"], edge_dtype=self._edge_key(),   # :70-73 + graph_model_base.py:97-127
                          virtual_edge_table=self._virtual_edge_table())

    def embeddings(self, node_features, feature_matrix, graph_matrix):
        """h [B,N,Dh] (real nodes: the virtual ones join after the positional encodings), e and mask with the virtual nodes"""
        h, mask = self._node_embedding(node_features)
        return h, self._edge_embedding(feature_matrix, graph_matrix), mask

    def _node_params(self):
        """(node_emb, node_emb_bias) as egt_amd.node_embed takes them"""
        return self.node_emb, None

    def _fused_node_input(self, node_features, singular_vectors=None, eigen_vectors=None, pe_signs=None):
        """(h [B,nv+N,Dh], mask [B,nv+N]) from the fused op (egt_amd.node_embed), or None where it does not apply: the tensors
        are fp32 on the GPU, the library covers the geometry (egt_node_embed_supported) and EGT_NO_NODE_EMBED is not set.  The
        sign sample of the random flip is drawn here with the expression `positional` uses, so a seeded run sees the same
        stream."""
        from .node_embed import draw_pe_signs, node_embed, node_embed_disabled, node_embed_supported
        c, nv = self.cfg, self.num_virtual_nodes
        kind = "svd" if c["use_svd"] else ("eig" if c["use_eig"] else None)
        pe = singular_vectors if kind == "svd" else (eigen_vectors if kind == "eig" else None)
        sel, transform = (c[f"sel_{kind}_features"], c[f"transform_{kind}"]) if kind else (0, False)
        emb, emb_bias = self._node_params()
        Dh = emb.shape[1]
        is_float = node_features.dtype.is_floating_point
        if not node_features.is_cuda or emb.dtype != torch.float32 or node_features.dim() != (3 if is_float else 2) \
                or node_embed_disabled():
            return None
        if kind is not None and not (pe is not None and pe.is_cuda and pe.dim() == (4 if kind == "svd" else 3) and
                                     (kind != "svd" or pe.shape[3] == 2) and pe.shape[:2] == node_features.shape[:2]):
            return None
        B, N = node_features.shape[:2]
        if not node_embed_supported(B, N, Dh, nv, 0 if is_float else emb.shape[0], node_features.shape[2] if is_float else 0,
                                    kind, pe.shape[2] if kind else 0, sel, transform):
            return None
        signs = None
        if kind is not None and c["random_neg"] and self.training:
            width = sel if transform else max(sel, Dh // 2 if kind == "svd" else Dh)      # (the untransformed encoding is zero-padded first)
            signs = pe_signs if pe_signs is not None else \
                draw_pe_signs((B, 1, width, 1) if kind == "svd" else (B, 1, width), node_features.device)
        return node_embed(node_features, emb, emb_bias, pe, kind, sel, self._pe_dense() if transform else None, signs,
                          self.virtual_node_emb if nv else None, getattr(self, "mask_value", -1.0))

    def node_input(self, node_features, singular_vectors=None, eigen_vectors=None, pe_signs=None):
        """(h [B,nv+N,Dh], mask [B,nv+N]): the node embedding, the positional encoding and the virtual rows -- ONE op where
        `_fused_node_input` applies, the composed ops otherwise"""
        out = self._fused_node_input(node_features, singular_vectors, eigen_vectors, pe_signs)
        if out is None:
            h, mask = self._node_embedding(node_features)
            out = self.with_virtual_nodes(self.positional(h, singular_vectors, eigen_vectors, pe_signs)), mask
        return out

    def inputs(self, node_features, feature_matrix, graph_matrix, singular_vectors=None, eigen_vectors=None, pe_signs=None):
        """(h [B,nv+N,Dh], e, mask) as they enter the layer stack: `node_input` and the edge embedding; where the fused node op
        does not apply, `embeddings` -> `positional` -> `with_virtual_nodes` as before"""
        out = self._fused_node_input(node_features, singular_vectors, eigen_vectors, pe_signs)
        if out is None:
            h, e, mask = self.embeddings(node_features, feature_matrix, graph_matrix)
            return self.with_virtual_nodes(self.positional(h, singular_vectors, eigen_vectors, pe_signs)), e, mask
        return out[0], self._edge_embedding(feature_matrix, graph_matrix), out[1]

    def distance_aux(self, e, graph_matrix):
        """{"distance_loss": per_graph [B]}: the distance objective on the final edge channels (graph_model_base.py:66-94)"""
        from .head import distance_target
        return {"distance_loss": self.dist_head(e, distance_target(graph_matrix, self.cfg["distance_target"]))}

    def _aux(self, y, e, graph_matrix, return_aux):
        if not return_aux:
            return y
        return y, (self.distance_aux(e, graph_matrix) if self.dist_head is not None else {})

    def forward(self, node_features, feature_matrix, graph_matrix, attn_mask=None, singular_vectors=None,
                eigen_vectors=None, pe_signs=None, return_aux=False):
        h, e, mask = self.inputs(node_features, feature_matrix, graph_matrix, singular_vectors, eigen_vectors, pe_signs)
        h, e = self.layers(h, e, mask, self.edge_mask(graph_matrix, attn_mask),
                           skip_last_edge_ffn=self.dist_head is None)                   # :336-341
        if self.node_norm_final is not None:
            h = self.node_norm_final(h)                                                 # :343-345
        x = self.graph_readout(h, mask)                                                 # zinc/dc.py:105-110
        for lyr in self.mlp_out:                                                        # mlp_out, :354-372
            x = lyr(x)
            x = F.elu(x) if self.cfg["activation"] == 'elu' else torch.relu(x)
        return self._aux(self.target(x), e, graph_matrix, return_aux)                   # zinc/dc.py:116-117

    GRAPH_LOSS = "mae"            # the loss of graph_loss: MeanAbsoluteError here, the sparse cross-entropy in the CIFAR10 / MNIST models

    def graph_head_params(self):
        """(gamma, beta, mlp_out kernels / biases ..., target kernel, target bias): the readout's parameters in the order
        egt_amd.graph_head takes them (gamma / beta None without node_norm_final)"""
        n = self.node_norm_final
        mid = [t for m in self.mlp_out for t in (m.kernel, m.bias)]
        return (None if n is None else n.gamma, None if n is None else n.beta, *mid, self.target.kernel, self.target.bias)

    def graph_head_fused(self, h) -> bool:
        """whether the readout + loss of a step run in the fused kernels: h [B,nv+N,Dh] is fp32 on the GPU, the library
        covers the geometry (egt_graph_head_supported) and EGT_NO_GRAPH_HEAD is not set"""
        from .graph_head import graph_head_disabled, graph_head_supported
        if not h.is_cuda or h.dtype != torch.float32 or len(self.mlp_out) != 2 or graph_head_disabled():
            return False
        nv = self.num_virtual_nodes
        return graph_head_supported(h.shape[0], h.shape[1] - nv, h.shape[2], self.mlp_out[0].kernel.shape[1],
                                    self.mlp_out[1].kernel.shape[1], self.target.kernel.shape[1], nv, self.GRAPH_LOSS,
                                    self.cfg["activation"], self.node_norm_final is not None)

    def graph_loss(self, node_features, feature_matrix, graph_matrix, target, attn_mask=None, singular_vectors=None,
                   eigen_vectors=None, pe_signs=None, return_aux=False):
        """The step's end of the model: embeddings, positional encodings, virtual nodes and layers as in `forward`, then
        node_norm_final, the pooling, the readout MLP, the loss and the metric sums as ONE op (egt_amd.graph_head: the fused
        kernels where they cover the geometry, the composed head otherwise).  Returns (loss, stats, pred, aux): stats =
        [sum |y - t|, 0, B C] (GRAPH_LOSS 'mae') or [sum CE, sum [argmax == t], B] ('xent'), loss = stats[0] / stats[2] (the
        Keras batch mean), pred [B,C] what `forward` returns (no gradient), aux as `forward(return_aux=True)` returns it."""
        from .graph_head import graph_head_composed, graph_head_loss
        h, e, mask = self.inputs(node_features, feature_matrix, graph_matrix, singular_vectors, eigen_vectors, pe_signs)
        h, e = self.layers(h, e, mask, self.edge_mask(graph_matrix, attn_mask), skip_last_edge_ffn=self.dist_head is None)
        head = graph_head_loss if self.graph_head_fused(h) else graph_head_composed
        stats, pred = head(h, target, mask, self.graph_head_params(), self.GRAPH_LOSS, self.num_virtual_nodes,
                           self.cfg["activation"])
        loss = stats[0] / stats[2].detach()
        aux = self.distance_aux(e, graph_matrix) if (return_aux and self.dist_head is not None) else {}
        return loss, stats, pred.detach(), aux


class _NotInherited:
    """a method of the graph-level models that a per-node model does not have (hasattr is False)"""

    def __set_name__(self, owner, name):
        self.name = name

    def __get__(self, obj, owner=None):
        raise AttributeError(f"{getattr(owner, '__name__', 'model')} has no {self.name}: its readout is per node (classification_loss)")


class PatternDCTransformer(ZincDCTransformer):
    """lib.models.sbm_pattern.dc.DCSVDTransformer for scheme pattern.svd (use_svd false): integer node features
    (3 values), the adjacency hop embedding as the ONLY edge-channel input (no feature matrix), per-node readout
    `mlp_out -> Dense(num_target_labels)` (sbm_pattern/dc.py:51-58).  edge_width 8 in the shipped configs."""
    HAS_VIRTUAL_NODES = False
    graph_head_params = _NotInherited()
    graph_head_fused = _NotInherited()
    graph_loss = _NotInherited()

    def __init__(self, num_node_features=3, num_target_labels=2, edge_width=8, model_height=16, **kw):
        kw.pop("num_edge_features", None); kw.pop("num_targets", None)
        super().__init__(num_node_features=num_node_features, num_edge_features=0, num_targets=num_target_labels,
                         edge_width=edge_width, model_height=model_height, **kw)
        # no fm_emb in this model: the embedding kernel gets a one-row ZERO table (a constant buffer, not a parameter)
        del self.fm_emb
        self.register_buffer("fm_emb", torch.zeros(1, edge_width), persistent=False)

    def keras_named_parameters(self):
        out = super().keras_named_parameters()
        out.pop("fm_emb/embeddings", None)
        return out

    def forward(self, node_features, graph_matrix, attn_mask=None, return_mask=False, singular_vectors=None,
                eigen_vectors=None, pe_signs=None, return_aux=False):
        fmat = torch.full(graph_matrix.shape, -1, dtype=torch.int32, device=graph_matrix.device)
        h, e, mask = self.inputs(node_features, fmat, graph_matrix, singular_vectors, eigen_vectors, pe_signs)
        h, e = self.layers(h, e, mask, self.edge_mask(graph_matrix, attn_mask), skip_last_edge_ffn=self.dist_head is None)
        if self.node_norm_final is not None:
            h = self.node_norm_final(h)
        x = h
        for lyr in self.mlp_out:
            x = lyr(x)
            x = F.elu(x) if self.cfg["activation"] == 'elu' else torch.relu(x)
        y = self.target(x)                                                                # logits [B,N,C]
        return self._aux((y, mask) if return_mask else y, e, graph_matrix, return_aux)

    def head_params(self):
        """(gamma, beta, mlp_out kernels / biases ..., target kernel, target bias): the readout's parameters in the order
        egt_amd.node_head takes them (gamma / beta None without node_norm_final)"""
        n = self.node_norm_final
        mid = [t for m in self.mlp_out for t in (m.kernel, m.bias)]
        return (None if n is None else n.gamma, None if n is None else n.beta, *mid, self.target.kernel, self.target.bias)

    def node_head_fused(self, h) -> bool:
        """whether the readout + loss of a training step run in the fused kernels: the tensors are on the GPU, the library
        covers the geometry (egt_node_head_supported) and EGT_NO_NODE_HEAD is not set"""
        from .node_head import node_head_disabled, node_head_supported
        if not h.is_cuda or h.dtype != torch.float32 or len(self.mlp_out) != 2 or node_head_disabled():
            return False
        return node_head_supported(h.shape[0], h.shape[1], h.shape[2], self.mlp_out[0].kernel.shape[1],
                                   self.mlp_out[1].kernel.shape[1], self.target.kernel.shape[1], self.cfg["activation"],
                                   self.node_norm_final is not None)

    def classification_loss(self, node_features, graph_matrix, target, class_weights, attn_mask=None, singular_vectors=None,
                            eigen_vectors=None, pe_signs=None, return_aux=False):
        """The training step's end of the model: embeddings, positional encodings and layers as in `forward`, then the
        readout, the class-weighted sparse cross-entropy and the metric sums as ONE op (egt_amd.node_head: the fused kernels
        where they cover the geometry, the composed head otherwise) -- no logits tensor.  Returns (loss, stats, aux):
        stats = [sum mask w[y] CE, sum mask [argmax == y], sum mask], loss = stats[0] / (B N) (Keras SUM_OVER_BATCH_SIZE
        counts the padded slots: weighted_sparse_xent_loss), aux as `forward(return_aux=True)` returns it."""
        from .node_head import node_head_composed, node_head_loss
        fmat = torch.full(graph_matrix.shape, -1, dtype=torch.int32, device=graph_matrix.device)
        h, e, mask = self.inputs(node_features, fmat, graph_matrix, singular_vectors, eigen_vectors, pe_signs)
        h, e = self.layers(h, e, mask, self.edge_mask(graph_matrix, attn_mask), skip_last_edge_ffn=self.dist_head is None)
        head = node_head_loss if self.node_head_fused(h) else node_head_composed
        stats = head(h, target, mask, class_weights, self.head_params(), self.cfg["activation"])
        loss = stats[0] / (h.shape[0] * h.shape[1])
        aux = self.distance_aux(e, graph_matrix) if (return_aux and self.dist_head is not None) else {}
        return loss, stats, aux


class ClusterDCTransformer(PatternDCTransformer):
    """lib.models.sbm_cluster.dc.DCSVDTransformer for the cluster.svd / cluster.eig schemes: the PATTERN model with seven
    node-feature values (0 = unlabelled, 1..6 = the labelled seed node of a community) and six target classes."""

    def __init__(self, num_node_features=7, num_target_labels=6, **kw):
        super().__init__(num_node_features=num_node_features, num_target_labels=num_target_labels, **kw)


class Cifar10DCTransformer(ZincDCTransformer):
    """lib.models.cifar10.dc.DCSVDTransformer for scheme cifar10.svd (use_svd false; the MNIST model has the same
    structure): real-valued node features [B,N,5] and edge features [B,N,N,1], each through keras Masking(mask_value)
    + Dense (cifar10/dc.py:66-73); the adjacency hop embedding is added to the edge embedding; graph-level readout
    (masked mean pool -> mlp_out -> Dense(num_target_labels)).  edge_width 8 / model_height 4 in the shipped config."""

    GRAPH_LOSS = "xent"

    def __init__(self, num_node_features=5, num_edge_features=1, num_target_labels=10, mask_value=-1., edge_width=8,
                 model_height=4, **kw):
        kw.pop("num_targets", None)
        super().__init__(num_node_features=1, num_edge_features=0, num_targets=num_target_labels,
                         edge_width=edge_width, model_height=model_height, **kw)
        del self.node_emb, self.fm_emb
        self.register_buffer("fm_emb", torch.zeros(1, edge_width), persistent=False)   # no integer feature matrix here
        self.mask_value = float(mask_value)
        self.node_emb = KerasDense(num_node_features, self.cfg["model_width"])
        self.edge_emb = KerasDense(num_edge_features, edge_width)

    def keras_named_parameters(self):
        out = super().keras_named_parameters()
        out.pop("fm_emb/embeddings", None); out.pop("node_emb/embeddings", None)
        out.update({"node_emb/kernel": self.node_emb.kernel, "node_emb/bias": self.node_emb.bias,
                    "edge_emb/kernel": self.edge_emb.kernel, "edge_emb/bias": self.edge_emb.bias})
        return out

    def _node_embedding(self, node_features):
        from .masks import node_mask_from_masking
        nv = self.num_virtual_nodes
        mask = node_mask_from_masking(node_features, self.mask_value, nv)               # keras Masking, cifar10/dc.py:68
        h = self.node_emb(node_features * mask[:, nv:, None].to(node_features.dtype))   # Masking zeroes the padded rows
        return h, mask

    def _edge_embedding(self, feature_matrix, graph_matrix):
        fmat = torch.full(graph_matrix.shape, -1, dtype=torch.int32, device=graph_matrix.device)
        return edge_embed(fmat, graph_matrix, self.fm_emb, self.adj_emb.kernel, self.adj_emb.bias,
                          clip_hops=self.cfg["clip_hops"], float_features=feature_matrix, float_kernel=self.edge_emb.kernel,
                          float_bias=self.edge_emb.bias, mask_value=self.mask_value,
                          edge_dtype=self._edge_key(),                                  # :71-73 + graph_model_base.py:97-127
                          virtual_edge_table=self._virtual_edge_table())

    def _node_params(self):
        return self.node_emb.kernel, self.node_emb.bias


class MnistDCTransformer(Cifar10DCTransformer):
    """lib.models.mnist.dc.DCSVDTransformer for scheme mnist.svd: the CIFAR10 model with three node features (grey level +
    x, y of a superpixel)."""
    HAS_VIRTUAL_NODES = False     # lib/models/mnist/dc.py has no VNModel

    def __init__(self, num_node_features=3, **kw):
        super().__init__(num_node_features=num_node_features, **kw)


def sparse_xent_loss(logits, y_true):
    """keras.losses.SparseCategoricalCrossentropy(from_logits=True) (schemes/cifar10/svd.py:37-40): batch mean."""
    return F.cross_entropy(logits, y_true.long())


def class_weights_from_sizes(class_sizes, device=None):
    """WeightedSparseXEntropyLoss (lib/base/genutil/losses.py:41-46)."""
    cs = torch.as_tensor(class_sizes, dtype=torch.float32, device=device)
    w = cs.sum() - cs
    return w / w.sum()


def weighted_sparse_xent_loss(logits, y_true, mask, class_weights):
    """schemes/pattern/svd.py:34-39: class-weighted sparse cross-entropy per node, masked by the node mask, divided by
    the number of (graph, node) slots (Keras SUM_OVER_BATCH_SIZE counts the padded slots too)."""
    logp = torch.log_softmax(logits, dim=-1)
    y = y_true.clamp(min=0).long()
    xent = -logp.gather(-1, y[..., None])[..., 0]
    per = class_weights[y] * xent * mask.to(logits.dtype)
    return per.sum() / per.numel()


def mae_loss(y_pred, y_true):
    """keras.losses.MeanAbsoluteError (schemes/zinc/svd.py:37-39)."""
    return (y_pred - y_true).abs().mean()
