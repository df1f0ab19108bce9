"""Readout and loss of the node-classification schemes (PATTERN, CLUSTER): ``mlp_out(h) -> Dense(num_target_labels)`` after
``node_norm_final`` (sbm_pattern/dc.py:51-58, sbm_cluster/dc.py), the class-weighted sparse cross-entropy and the sums
the metrics need, over the R = B N rows of h [B,N,W]:

    z     = Dense_t(act(Dense_1(act(Dense_0(node_norm_final(h))))))
    stats = [ sum mask w[y] CE(z, y),   sum mask [argmax z == y],   sum mask ]                lib/base/genutil/losses.py:41-118

On the GPU this is one kernel per direction (egt_node_head_fwd / egt_node_head_bwd, egt_amd/csrc/egt_head.hip): h is read
once forward, h read and d_h written once backward, no logits tensor, nothing row-sized kept between them.
`node_head_composed` is the same from torch ops: the A/B baseline of tools/bench_node_head.py, the route of geometries the
kernels do not cover, and the CPU path.  EGT_NO_NODE_HEAD=1 (read once per process) keeps the composed head everywhere.
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

_NO_NODE_HEAD = None


def node_head_disabled() -> bool:
    """EGT_NO_NODE_HEAD=1 (read once per process): the models keep the composed head."""
    global _NO_NODE_HEAD
    if _NO_NODE_HEAD is None:
        _NO_NODE_HEAD = os.environ.get("EGT_NO_NODE_HEAD", "") not in ("", "0")
    return _NO_NODE_HEAD


def node_head_desc(B, N, W, M0, M1, C_, activation="elu", layernorm=True, eps=LN_EPS) -> L.NodeHeadDesc:
    return L.NodeHeadDesc(B=B, N=N, W=W, M0=M0, M1=M1, C=C_, activation=_ACT.get(activation, L.ACT_NONE),
                          flags=L.NH_LAYERNORM if layernorm else 0, ln_eps=eps, reserved=0)


def node_head_supported(B, N, W, M0, M1, C_, activation="elu", layernorm=True) -> bool:
    """the library's answer (egt_node_head_supported) for a geometry"""
    return bool(L.load().egt_node_head_supported(C.byref(node_head_desc(B, N, W, M0, M1, C_, activation, layernorm))))


def node_head_composed(h, target, mask, class_weights, params, activation="elu", eps=LN_EPS):
    """The head, its loss and the metric sums from plain torch ops (any device, any float dtype of the parameters).
    params: (gamma, beta, W0, b0, W1, b1, Wt, bt), gamma / beta None without node_norm_final.  Returns stats [3]; only
    stats[0] carries a gradient."""
    gamma, beta, *mid, Wt, bt = params            # (any number of hidden Dense layers; the kernels cover two)
    act = F.elu if activation == "elu" else torch.relu
    x = h.to(Wt.dtype)
    if gamma is not None:
        x = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    x = x.reshape(-1, x.shape[-1])
    for k, b in zip(mid[0::2], mid[1::2]):
        x = act(torch.addmm(b, x, k))
    z = torch.addmm(bt, x, Wt)
    m = mask.reshape(-1).to(z.dtype)
    y = target.reshape(-1).clamp(min=0, max=z.shape[-1] - 1).long()     # (a masked slot's target is never a class)
    xent = -torch.log_softmax(z, dim=-1).gather(-1, y[:, None])[:, 0]
    loss = (class_weights.to(z.dtype)[y] * xent * m).sum()
    hit = ((z.detach().argmax(-1) == target.reshape(-1)).to(z.dtype) * m).sum()
    return torch.stack([loss, hit, m.sum()])


class _FusedNodeHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, target, mask, class_weights, desc, *params):
        _need_gpu(h, target, mask, class_weights)
        lib = L.load()
        h = _f32c(h)
        ctx.param_objs = params
        params = tuple(None if p is None else _f32c(p) for p in params)
        stats = torch.empty(3, dtype=torch.float32, device=h.device)
        ws = torch.empty(lib.egt_node_head_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=h.device)
        pst = L.params_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, params)
        L.check(lib.egt_node_head_fwd(C.byref(desc), C.byref(pst), L.ptr(h), L.ptr(target), L.ptr(mask), L.ptr(class_weights),
                                      L.ptr(stats), L.ptr(ws), L.current_stream()))
        ctx.desc = desc
        ctx.has_ln = params[0] is not None
        ctx.save_for_backward(h, target, mask, class_weights, *[p for p in params if p is not None])
        return stats

    @staticmethod
    def backward(ctx, d_stats):
        lib = L.load()
        h, target, mask, class_weights, *params = ctx.saved_tensors
        if not ctx.has_ln:
            params = [None, None] + params
        desc = ctx.desc
        s = _f32c(d_stats.to(torch.float32))        # element 0 is the upstream gradient of the loss sum: read on the device
        dh = torch.empty_like(h)
        from .fused import grad_sinks
        grads, rets = grad_sinks(ctx.param_objs)
        ws = torch.empty(lib.egt_node_head_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=h.device)
        pst, gst = (L.params_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, t) for t in (params, grads))
        L.check(lib.egt_node_head_bwd(C.byref(desc), C.byref(pst), L.ptr(h), L.ptr(target), L.ptr(mask), L.ptr(class_weights),
                                      L.ptr(s), L.ptr(dh), C.byref(gst), L.ptr(ws), L.current_stream()))
        return (dh, None, None, None, None, *rets)


def node_head_loss(h, target, mask, class_weights, params, activation="elu", eps=LN_EPS):
    """Fused head + loss + metric sums: h [B,N,W] fp32, target [B,N] integer classes, mask [B,N] bool, class_weights [C],
    params as in node_head_composed -> stats [3] fp32 (only stats[0] is differentiable).  Raises for a geometry the kernels
    do not cover: the caller asks node_head_supported first."""
    gamma, beta, W0, b0, W1, b1, Wt, bt = params
    B, N, W = h.shape
    desc = node_head_desc(B, N, W, W0.shape[1], W1.shape[1], Wt.shape[1], activation, gamma is not None, eps)
    if not L.load().egt_node_head_supported(C.byref(desc)):
        raise ValueError(f"node head kernel covers W in 16/32/48/64, hidden widths (24,12)/(32,16), 2..16 classes, elu/relu; got "
                         f"W={W}, hidden ({W0.shape[1]},{W1.shape[1]}), {Wt.shape[1]} classes, {activation!r}")
    if tuple(target.shape) != (B, N) or tuple(mask.shape) != (B, N) or target.dtype.is_floating_point:
        raise TypeError("node head: target must be an integer [B,N] tensor and mask a [B,N] tensor")
    if class_weights.numel() != Wt.shape[1]:
        raise ValueError(f"node head: {class_weights.numel()} class weights for {Wt.shape[1]} classes")
    target = target.to(torch.int32).contiguous()
    return _FusedNodeHead.apply(h, target, _u8c(mask), _f32c(class_weights.to(torch.float32)), desc, *params)
