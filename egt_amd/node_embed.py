"""Node input of every model: from a batch's node features to the h [B,nv+N,Dh] and mask [B,nv+N] that enter the layer stack

    row nv+n = node_emb[features + 1]                       integer features, padding -1 (masking.py:31-43)
               Dense(Masking(mask_value)(features))         float feature rows (cifar10/dc.py:66-69)
             + the SVD / eigenvector encoding               SVDFeatModel / EigFeatModel (graph_model_base.py:284-414)
    rows 0..nv-1 = virtual_node_emb                         VNModel.combine_node_embeddings (graph_model_base.py:227-235)

On the GPU this is one launch forward and two backward (egt_node_embed_fwd / egt_node_embed_bwd,
egt_amd/csrc/egt_node_embed.hip).  `node_embed_composed` is the same from torch ops: the A/B baseline of
tools/bench_node_embed.py, the route of geometries the kernels do not cover, and the CPU path.  EGT_NO_NODE_EMBED=1 (read once
per process) keeps the composed ops everywhere.  The sign sample of the training-time flip (RandomNeg / RandomNegEig,
misc.py:53-94) is an input of both: the model draws it (`draw_pe_signs`).
"""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.nn.functional as F

from . import _lib as L
from .functional import _f32c, _need_gpu

_PE = {None: L.NE_PE_NONE, "svd": L.NE_PE_SVD, "eig": L.NE_PE_EIG}

_NO_NODE_EMBED = None


def node_embed_disabled() -> bool:
    """EGT_NO_NODE_EMBED=1 (read once per process): the models keep the composed ops."""
    global _NO_NODE_EMBED
    if _NO_NODE_EMBED is None:
        _NO_NODE_EMBED = os.environ.get("EGT_NO_NODE_EMBED", "") not in ("", "0")
    return _NO_NODE_EMBED


def node_embed_desc(B, N, Dh, nv=0, R=0, F_=0, pe_kind=None, T=0, sel=0, transform=False, signs=False, mask_value=-1.0,
                    sign_stride=0) -> L.NodeEmbedDesc:
    """R > 0: integer features and a table of R rows; F_ > 0: float feature rows of F_ columns.  pe_kind None / 'svd' / 'eig'.
    An unknown pe_kind gives a descriptor the library refuses."""
    flags = (L.NE_TRANSFORM if transform else 0) | (L.NE_SIGNS if signs else 0)
    return L.NodeEmbedDesc(B=B, N=N, Dh=Dh, nv=nv, kind=L.NE_FLOAT if F_ else L.NE_INT, R=R, F=F_, pe_kind=_PE.get(pe_kind, -1), T=T,
                           sel=sel, flags=flags, mask_value=float(mask_value), sign_stride=sign_stride, reserved=0)


def node_embed_supported(B, N, Dh, nv=0, R=0, F_=0, pe_kind=None, T=0, sel=0, transform=False) -> bool:
    """the library's answer (egt_node_embed_supported) for a geometry"""
    return bool(L.load().egt_node_embed_supported(C.byref(node_embed_desc(B, N, Dh, nv, R, F_, pe_kind, T, sel, transform))))


def draw_pe_signs(shape, device):
    """one sign per (graph, feature) of the random flip, as the models have always drawn it"""
    return torch.where(torch.rand(*shape, device=device) < 0.5, -1.0, 1.0)


def _dense(x, kernel, bias):
    """KerasDense.forward: on the GPU one library GEMM with the bias in its epilogue"""
    if x.is_cuda and x.dim() >= 2 and x.dtype == kernel.dtype:
        return torch.addmm(bias, x.reshape(-1, x.shape[-1]), kernel).view(*x.shape[:-1], kernel.shape[1])
    return x @ kernel + bias


def positional_composed(h, pe, pe_kind, sel, transform, dense=None, signs=None, draw=False):
    """h + the SVD ('svd': pe [B,N,T,2]) / eigenvector ('eig': pe [B,N,T]) embedding of its first `sel` features.  signs
    ([B,1,F,1] / [B,1,F], F the feature count after the zero padding of the untransformed encoding) is the sample of the sign
    flip; draw: sample it here when none is given.  dense = (kernel, bias) of svd_emb / eig_emb under `transform`."""
    Dh = h.shape[-1]
    if pe_kind == "svd":
        v = pe.to(h.dtype)[:, :, :sel, :]
        if not transform:
            v = F.pad(v, (0, 0, 0, max(0, Dh // 2 - sel)))
        if signs is not None or draw:
            sg = signs if signs is not None else draw_pe_signs((v.shape[0], 1, v.shape[2], 1), v.device)
            v = v * sg.to(v.dtype)
        v = torch.cat(torch.unbind(v, dim=-1), dim=-1)
    else:
        v = pe.to(h.dtype)[:, :, :sel]
        if not transform:
            v = F.pad(v, (0, max(0, Dh - sel)))
        if signs is not None or draw:
            sg = signs if signs is not None else draw_pe_signs((v.shape[0], 1, v.shape[2]), v.device)
            v = v * sg.to(v.dtype)
    if transform:
        v = _dense(v, *dense)
    return h + v


def virtual_rows_composed(h, virtual_node_emb):
    """[B,N,Dh] -> [B,nv+N,Dh]: the virtual-node embeddings in front of every graph's nodes"""
    return torch.cat([virtual_node_emb.to(h.dtype)[None].expand(h.shape[0], -1, -1), h], dim=1)


def node_embed_composed(features, node_emb, node_emb_bias=None, pe=None, pe_kind=None, sel=0, pe_dense=None, signs=None,
                        virtual_node_emb=None, mask_value=-1.0):
    """The node input from plain torch ops (any device, any float dtype of the parameters) -> (h [B,nv+N,Dh], mask bool).
    Integer features [B,N] with the table node_emb [R,Dh], or float rows [B,N,F] with the Dense (node_emb [F,Dh],
    node_emb_bias); pe_dense = (kernel, bias) or None (the encoding is added to its channels); signs as positional_composed
    takes them, or None for no flip."""
    if features.dtype.is_floating_point:
        real = (features != mask_value).any(dim=-1)
        x = (features * real[..., None].to(features.dtype)).to(node_emb.dtype)
        h = _dense(x, node_emb, node_emb_bias)
    else:
        real = features != -1
        h = F.embedding((features + 1).long(), node_emb)
    if pe_kind is not None:
        h = positional_composed(h, pe, pe_kind, sel, pe_dense is not None, pe_dense, signs)
    if virtual_node_emb is not None and virtual_node_emb.shape[0]:
        h = virtual_rows_composed(h, virtual_node_emb)
        real = torch.cat([torch.ones(real.shape[0], virtual_node_emb.shape[0], dtype=torch.bool, device=real.device), real], dim=1)
    return h, real


class _FusedNodeEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, pe, signs, desc, *params):
        """params: (node_emb, node_emb_bias, pe_kernel, pe_bias, virtual_node_emb), None where the geometry has none"""
        _need_gpu(features, pe, signs)
        lib = L.load()
        ctx.param_objs = params
        tensors = tuple(None if p is None else _f32c(p) for p in params)
        h = torch.empty(desc.B, desc.nv + desc.N, desc.Dh, dtype=torch.float32, device=features.device)
        mask = torch.empty(desc.B, desc.nv + desc.N, dtype=torch.bool, device=features.device)   # one 0 / 1 byte per element
        pst = L.params_struct(L.NodeEmbedParams, L.NODE_EMBED_PARAM_FIELDS, tensors)
        L.check(lib.egt_node_embed_fwd(C.byref(desc), C.byref(pst), L.ptr(features), L.ptr(pe), L.ptr(signs), L.ptr(h), L.ptr(mask),
                                       L.current_stream()))
        ctx.desc = desc
        ctx.save_for_backward(features, pe, signs)
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)           # (no zeros tensor, and its fill launch, for the mask's absent gradient)
        return h, mask

    @staticmethod
    def backward(ctx, d_h, _d_mask):
        lib = L.load()
        features, pe, signs = ctx.saved_tensors
        desc = ctx.desc
        if d_h is None:
            return (None,) * (4 + len(ctx.param_objs))
        d_h = _f32c(d_h.to(torch.float32))
        from .fused import grad_sinks
        grads, rets = grad_sinks(ctx.param_objs)
        ws = torch.empty(lib.egt_node_embed_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=d_h.device)
        gst = L.params_struct(L.NodeEmbedParams, L.NODE_EMBED_PARAM_FIELDS, grads)
        L.check(lib.egt_node_embed_bwd(C.byref(desc), L.ptr(features), L.ptr(pe), L.ptr(signs), L.ptr(d_h), C.byref(gst), L.ptr(ws),
                                       L.current_stream()))
        return (None, None, None, None, *rets)


def node_embed(features, node_emb, node_emb_bias=None, pe=None, pe_kind=None, sel=0, pe_dense=None, signs=None,
               virtual_node_emb=None, mask_value=-1.0):
    """Fused node input: the arguments of node_embed_composed, fp32 on the GPU -> (h [B,nv+N,Dh] fp32, mask [B,nv+N] bool).
    signs: [B, >= sel] floats of +-1 (any shape whose per-graph stride holds the features' signs first: the model's
    [B,1,F,1] / [B,1,F] sample) or None.  Raises for a geometry the kernels do not cover: the caller asks
    node_embed_supported first."""
    B, N = features.shape[:2]
    Dh = node_emb.shape[1]
    nv = 0 if virtual_node_emb is None else int(virtual_node_emb.shape[0])
    if features.dtype.is_floating_point:
        R, F_ = 0, int(features.shape[2])
        features = _f32c(features.to(torch.float32))
    else:
        R, F_ = int(node_emb.shape[0]), 0
        features = features.to(torch.int32).contiguous()
    T = stride = 0
    if pe_kind is not None:
        pe = _f32c(pe.to(torch.float32))              # [B,N,T,2] / [B,N,T]: wider than what is used; the kernel strides over it
        T = int(pe.shape[2])
        if signs is not None:
            signs = _f32c(signs.to(torch.float32)).reshape(B, -1)
            stride = int(signs.shape[1])
    else:
        pe = signs = None
    desc = node_embed_desc(B, N, Dh, nv, R, F_, pe_kind, T, sel, pe_dense is not None, signs is not None, mask_value, stride)
    if not L.load().egt_node_embed_supported(C.byref(desc)):
        raise ValueError(f"node embedding kernel covers Dh in 16/32/48/64, tables of up to 32 rows, up to 8 float features, up to 32 "
                         f"selected encoding features, 0..16 virtual nodes; got Dh={Dh}, R={R}, F={F_}, pe={pe_kind!r} sel={sel} of "
                         f"T={T}, transform={pe_dense is not None}, nv={nv}")
    kernel, bias = pe_dense if pe_dense is not None else (None, None)
    return _FusedNodeEmbed.apply(features, pe, signs, desc, node_emb, node_emb_bias, kernel, bias, virtual_node_emb if nv else None)
