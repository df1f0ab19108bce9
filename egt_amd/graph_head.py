"""Readout and loss of the graph-level schemes (zinc.svd / zinc.eig, zinc_full.*, cifar10.svd, mnist.svd): after
``node_norm_final`` the masked mean over the nodes (zinc/dc.py:109) -- or the virtual nodes' rows flattened (:105-108) --,
``mlp_out -> Dense(target)``, the loss and the sums the metrics need, over h [B,N',W] (N' = nv + N):

    y     = Dense_t(act(Dense_1(act(Dense_0(pool(node_norm_final(h)))))))
    MAE :  stats = [ sum |y - t|,   0,                       B C ]      t [B,C] float     schemes/zinc/svd.py:37-42
    XENT:  stats = [ sum CE(y, t),  sum [argmax y == t],     B   ]      t [B] integer     schemes/cifar10/svd.py:37-48

On the GPU this is one kernel per direction plus one small fixed-order reduction (egt_graph_head_fwd / egt_graph_head_bwd,
egt_amd/csrc/egt_graph_head.hip): h is read once forward, h read and d_h written once backward, nothing kept between them.
`graph_head_composed` is the same from torch ops: the A/B baseline of tools/bench_graph_head.py, the route of geometries the
kernels do not cover, and the CPU path.  EGT_NO_GRAPH_HEAD=1 (read once per process) keeps the composed head everywhere.
"""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.nn.functional as F

from . import _lib as L
from .functional import _f32c, _need_gpu, _u8c
from .layers import LN_EPS

_ACT = {"relu": L.ACT_RELU, "elu": L.ACT_ELU}
_LOSS = {"mae": L.GH_MAE, "xent": L.GH_XENT}

_NO_GRAPH_HEAD = None


def graph_head_disabled() -> bool:
    """EGT_NO_GRAPH_HEAD=1 (read once per process): the models keep the composed head."""
    global _NO_GRAPH_HEAD
    if _NO_GRAPH_HEAD is None:
        _NO_GRAPH_HEAD = os.environ.get("EGT_NO_GRAPH_HEAD", "") not in ("", "0")
    return _NO_GRAPH_HEAD


def graph_head_desc(B, N, W, M0, M1, C_, nv=0, loss="mae", activation="elu", layernorm=True, eps=LN_EPS) -> L.GraphHeadDesc:
    """N counts the real (padded) nodes: h has nv + N rows per graph.  An unknown loss / activation name gives a descriptor
    the library refuses."""
    return L.GraphHeadDesc(B=B, N=N, W=W, M0=M0, M1=M1, C=C_, nv=nv, loss=_LOSS.get(loss, -1),
                           activation=_ACT.get(activation, L.ACT_NONE), flags=L.GH_LAYERNORM if layernorm else 0, ln_eps=eps,
                           reserved=0)


def graph_head_supported(B, N, W, M0, M1, C_, nv=0, loss="mae", activation="elu", layernorm=True) -> bool:
    """the library's answer (egt_graph_head_supported) for a geometry"""
    return bool(L.load().egt_graph_head_supported(C.byref(graph_head_desc(B, N, W, M0, M1, C_, nv, loss, activation, layernorm))))


def graph_head_composed(h, target, mask, params, loss="mae", nv=0, activation="elu", eps=LN_EPS):
    """The head, its loss and the metric sums from plain torch ops (any device, any float dtype of the parameters).
    params: (gamma, beta, W0, b0, W1, b1, Wt, bt), gamma / beta None without node_norm_final.  Returns (stats [3], pred [B,C]);
    only stats[0] carries a gradient."""
    gamma, beta, *mid, Wt, bt = params            # (any number of hidden Dense layers; the kernels cover two)
    act = F.elu if activation == "elu" else torch.relu
    x = h.to(Wt.dtype)
    if gamma is not None:
        x = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    if nv:
        x = x[:, :nv].reshape(x.shape[0], nv * x.shape[2])
    else:
        m = mask.to(torch.bool)[..., None]
        x = torch.where(m, x, torch.zeros((), dtype=x.dtype, device=x.device)).sum(dim=1) / m.to(x.dtype).sum(dim=1)
    for k, b in zip(mid[0::2], mid[1::2]):
        x = act(torch.addmm(b, x, k))
    y = torch.addmm(bt, x, Wt)
    n = y.shape[0]
    if loss == "mae":
        t = target.to(y.dtype).reshape(n, -1)
        stats = [(y - t).abs().sum(), torch.zeros((), dtype=y.dtype, device=y.device),
                 torch.full((), float(t.numel()), dtype=y.dtype, device=y.device)]
    elif loss == "xent":
        t = target.reshape(n)
        tc = t.clamp(min=0, max=y.shape[-1] - 1).long()
        xent = -torch.log_softmax(y, dim=-1).gather(-1, tc[:, None])[:, 0]
        stats = [xent.sum(), (y.detach().argmax(-1) == t).to(y.dtype).sum(),
                 torch.full((), float(n), dtype=y.dtype, device=y.device)]
    else:
        raise ValueError(f"graph head: loss is 'mae' or 'xent' (got {loss!r})")
    return torch.stack(stats), y


class _FusedGraphHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, target, mask, desc, *params):
        _need_gpu(h, target, mask)
        lib = L.load()
        h = _f32c(h)
        if h.data_ptr() % 16:                       # (a view at an odd offset: the kernels load rows of h 16 bytes at a time)
            h = h.clone()
        ctx.param_objs = params
        params = tuple(None if p is None else _f32c(p) for p in params)
        stats = torch.empty(3, dtype=torch.float32, device=h.device)
        pred = torch.empty(desc.B, desc.C, dtype=torch.float32, device=h.device)
        ws = torch.empty(lib.egt_graph_head_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=h.device)
        pst = L.params_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, params)
        L.check(lib.egt_graph_head_fwd(C.byref(desc), C.byref(pst), L.ptr(h), L.ptr(target), L.ptr(mask), L.ptr(stats), L.ptr(pred),
                                       L.ptr(ws), L.current_stream()))
        ctx.desc = desc
        ctx.has_ln = params[0] is not None
        ctx.save_for_backward(h, target, mask, *[p for p in params if p is not None])
        ctx.mark_non_differentiable(pred)
        return stats, pred

    @staticmethod
    def backward(ctx, d_stats, _d_pred):
        lib = L.load()
        h, target, mask, *params = ctx.saved_tensors
        if not ctx.has_ln:
            params = [None, None] + params
        desc = ctx.desc
        s = _f32c(d_stats.to(torch.float32))        # element 0 is the upstream gradient of the loss sum: read on the device
        dh = torch.empty_like(h)
        from .fused import grad_sinks
        grads, rets = grad_sinks(ctx.param_objs)
        ws = torch.empty(lib.egt_graph_head_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=h.device)
        pst, gst = (L.params_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, t) for t in (params, grads))
        L.check(lib.egt_graph_head_bwd(C.byref(desc), C.byref(pst), L.ptr(h), L.ptr(target), L.ptr(mask), L.ptr(s), L.ptr(dh),
                                       C.byref(gst), L.ptr(ws), L.current_stream()))
        return (dh, None, None, None, *rets)


def graph_head_loss(h, target, mask, params, loss="mae", nv=0, activation="elu", eps=LN_EPS):
    """Fused head + loss + metric sums: h [B,nv+N,W] fp32, mask [B,nv+N] bool, target [B,C] float ('mae') or [B] integer
    classes ('xent'), params as in graph_head_composed -> (stats [3] fp32, pred [B,C] fp32); only stats[0] is
    differentiable.  Raises for a geometry the kernels do not cover: the caller asks graph_head_supported first."""
    gamma, beta, W0, b0, W1, b1, Wt, bt = params
    B, NP, W = h.shape
    Cc = Wt.shape[1]
    desc = graph_head_desc(B, NP - nv, W, W0.shape[1], W1.shape[1], Cc, nv, loss, activation, gamma is not None, eps)
    if not L.load().egt_graph_head_supported(C.byref(desc)):
        raise ValueError(f"graph head kernel covers W in 48/64, hidden widths (24,12)/(32,16), 1..16 outputs, 0..4 virtual nodes, "
                         f"elu/relu, 'mae'/'xent'; got W={W}, hidden ({W0.shape[1]},{W1.shape[1]}), {Cc} outputs, nv={nv}, "
                         f"{activation!r}, {loss!r}")
    if W0.shape[0] != max(nv, 1) * W or tuple(mask.shape) != (B, NP):
        raise AssertionError(f"graph head: mlp_out_0 kernel has {W0.shape[0]} rows for nv={nv}, W={W}; mask {tuple(mask.shape)} "
                             f"for h {tuple(h.shape)}")
    if loss == "mae":
        if target.numel() != B * Cc or not target.dtype.is_floating_point:
            raise TypeError(f"graph head: the 'mae' target is a float [B,C] tensor (got {tuple(target.shape)} {target.dtype})")
        target = _f32c(target.to(torch.float32).reshape(B, Cc))
    else:
        if target.numel() != B or target.dtype.is_floating_point:
            raise TypeError(f"graph head: the 'xent' target is an integer [B] tensor (got {tuple(target.shape)} {target.dtype})")
        target = target.reshape(B).to(torch.int32).contiguous()
    return _FusedGraphHead.apply(h, target, _u8c(mask), desc, *params)
