"""Distance objective of the reference's ``*_spe_do`` configs (``distance_loss`` / ``distance_target``): an auxiliary loss
over the FINAL edge channels e [B,N,N,De].

    target    = round(sum_{k=1..T} hop_k),  hop_1 = A,  hop_k = clip(A @ hop_{k-1}, 0, 1)      graph_model_base.py:66-76
    logits    = Dense_t(act(Dense_1(act(Dense_0(edge_norm_final(e))))))                       :83-94, xformer :343-372
    per_graph = sum_ij CE(logits, target) * (target > 0)                                      loss_layers.py:38-67

On the GPU the target is one kernel (egt_distance_target) and the head + loss one kernel per direction
(egt_edge_head_fwd / egt_edge_head_bwd, egt_amd/csrc/egt_head.hip): e is read once forward, e read and d_e written once
backward; nothing pair-sized is kept between them.  `distance_head_composed` is the same head from torch ops: the A/B
baseline of tools/bench_distance_head.py and the CPU restatement's counterpart -- GPU models always use the kernel.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
import torch.nn.functional as F

from . import _lib as L
from .functional import _f32c, _need_gpu
from .layers import KerasDense, KerasLayerNorm, LN_EPS

_ACT = {"relu": L.ACT_RELU, "elu": L.ACT_ELU}
_DTYPE = {torch.float32: L.EGT_F32, torch.bfloat16: L.EGT_BF16}


def head_desc(B, N, De, M0, M1, C_, activation="elu", layernorm=True, dtype=torch.float32, eps=LN_EPS) -> L.HeadDesc:
    if activation not in _ACT:
        raise ValueError(f"distance head activation must be one of {sorted(_ACT)} (got {activation!r})")
    if dtype not in _DTYPE:
        raise TypeError(f"distance head takes fp32 or bf16 edge tensors (got {dtype})")
    return L.HeadDesc(B=B, N=N, De=De, M0=M0, M1=M1, C=C_, dtype=_DTYPE[dtype], activation=_ACT[activation],
                      flags=L.EH_LAYERNORM if layernorm else 0, ln_eps=eps, reserved=0)


def distance_target(adj, T: int):
    """adj [B,N,N] -> uint8 [B,N,N]: how many of the first T clipped hop matrices connect the pair (the clip is applied
    whatever clip_hops says, and T is independent of upto_hop: graph_model_base.py:66-76)."""
    if adj.is_cuda:
        lib = L.load()
        adj = _f32c(adj.to(torch.float32))
        B, N, _ = adj.shape
        out = torch.empty(B, N, N, dtype=torch.uint8, device=adj.device)
        L.check(lib.egt_distance_target(L.ptr(adj), B, N, int(T), L.ptr(out), L.current_stream()))
        return out
    a = adj.to(torch.float64)
    hop, tot = a, a.clone()
    for _ in range(1, int(T)):
        hop = (a @ hop).clamp(0, 1)
        tot = tot + hop
    return tot.round().to(torch.uint8)


def distance_head_composed(e, target, params, activation="elu", eps=LN_EPS):
    """The head and its loss from plain torch ops (any device, any float dtype of the parameters).
    params: (gamma, beta, W0, b0, W1, b1, Wt, bt), gamma / beta None without edge_norm_final.  Returns per_graph [B]."""
    gamma, beta, W0, b0, W1, b1, Wt, bt = params
    act = F.elu if activation == "elu" else torch.relu
    x = e.to(W0.dtype)
    if gamma is not None:
        x = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    x = act(x @ W0 + b0)
    x = act(x @ W1 + b1)
    logp = torch.log_softmax(x @ Wt + bt, dim=-1)
    t = target.long()
    ce = -logp.gather(-1, t[..., None])[..., 0]
    return (ce * (t > 0).to(ce.dtype)).sum(dim=(1, 2))


class _FusedHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, target, desc, *params):
        _need_gpu(e, target)
        lib = L.load()
        if _DTYPE.get(e.dtype) != desc.dtype:
            raise TypeError(f"distance head: the descriptor's dtype is {desc.dtype}, e is {e.dtype}")
        e = e.contiguous()
        target = target.contiguous()
        ctx.param_objs = params
        params = tuple(None if p is None else _f32c(p) for p in params)
        per_graph = torch.empty(desc.B, dtype=torch.float32, device=e.device)
        ws = torch.empty(lib.egt_edge_head_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=e.device)
        pst = L.params_struct(L.HeadParams, L.HEAD_PARAM_FIELDS, params)
        L.check(lib.egt_edge_head_fwd(C.byref(desc), C.byref(pst), L.ptr(e), L.ptr(target), L.ptr(per_graph), L.ptr(ws),
                                      L.current_stream()))
        ctx.desc = desc
        ctx.has_ln = params[0] is not None
        ctx.save_for_backward(e, target, *[p for p in params if p is not None])
        return per_graph

    @staticmethod
    def backward(ctx, d_per_graph):
        lib = L.load()
        e, target, *params = ctx.saved_tensors
        if not ctx.has_ln:
            params = [None, None] + params
        desc = ctx.desc
        s = _f32c(d_per_graph.to(torch.float32))
        de = torch.empty_like(e)
        from .fused import grad_sinks
        grads, rets = grad_sinks(ctx.param_objs)
        ws = torch.empty(lib.egt_edge_head_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=e.device)
        pst, gst = (L.params_struct(L.HeadParams, L.HEAD_PARAM_FIELDS, t) for t in (params, grads))
        L.check(lib.egt_edge_head_bwd(C.byref(desc), C.byref(pst), L.ptr(e), L.ptr(target), L.ptr(s), L.ptr(de),
                                      C.byref(gst), L.ptr(ws), L.current_stream()))
        return (de, None, None, *rets)


def distance_head(e, target, params, activation="elu", eps=LN_EPS):
    """Fused head + loss: e [B,N,N,De] (fp32 / bf16), target uint8 [B,N,N], params as in distance_head_composed ->
    per_graph [B] fp32.  Raises for a geometry the kernels do not cover (there is no composed fallback)."""
    gamma, beta, W0, b0, W1, b1, Wt, bt = params
    B, N, _, De = e.shape
    desc = head_desc(B, N, De, W0.shape[1], W1.shape[1], Wt.shape[1], activation, gamma is not None, e.dtype, eps)
    if not L.load().egt_edge_head_supported(C.byref(desc)):
        raise ValueError(f"distance head kernel covers De in 8/16/32/48/64, hidden widths (24,12)/(32,16), 2..16 classes; got "
                         f"De={De}, hidden ({W0.shape[1]},{W1.shape[1]}), {Wt.shape[1]} classes, {e.dtype}")
    if target.dtype != torch.uint8 or tuple(target.shape) != (B, N, N):
        raise TypeError("distance head: target must be uint8 [B,N,N] (distance_target)")
    return _FusedHead.apply(e, target, desc, *params)


class DistanceHead(nn.Module):
    """edge_norm_final -> mlp_out_dist_targ_0 -> mlp_out_dist_targ_1 -> distance_target with the masked sparse
    cross-entropy summed per graph.  forward(e, target) -> per_graph [B]."""

    def __init__(self, edge_width, model_width, distance_target=8, mlp_layers=(.5, .25), activation="elu",
                 do_final_norm=True, edge_dtype=torch.float32):
        super().__init__()
        if len(mlp_layers) != 2:
            raise NotImplementedError("distance head is built for two hidden layers (mlp_layers = [.5, .25])")
        m0, m1 = (round(f * model_width) for f in mlp_layers)
        self.activation, self.num_classes = activation, int(distance_target) + 1
        desc = head_desc(1, 16, edge_width, m0, m1, self.num_classes, activation, do_final_norm, edge_dtype)
        if not L.load().egt_edge_head_supported(C.byref(desc)):
            raise NotImplementedError(f"distance head kernel does not cover edge_width={edge_width}, hidden widths ({m0},{m1}), "
                                      f"{self.num_classes} classes, {edge_dtype}")
        self.edge_norm_final = KerasLayerNorm(edge_width) if do_final_norm else None
        self.mlp_out_dist_targ = nn.ModuleList([KerasDense(edge_width, m0), KerasDense(m0, m1)])
        self.distance_target = KerasDense(m1, self.num_classes)

    def params(self):
        n = self.edge_norm_final
        d0, d1 = self.mlp_out_dist_targ
        return (None if n is None else n.gamma, None if n is None else n.beta, d0.kernel, d0.bias, d1.kernel, d1.bias,
                self.distance_target.kernel, self.distance_target.bias)

    def keras_named_parameters(self):
        out = {}
        if self.edge_norm_final is not None:
            out["edge_norm_final/gamma"], out["edge_norm_final/beta"] = self.edge_norm_final.gamma, self.edge_norm_final.beta
        for i, m in enumerate(self.mlp_out_dist_targ):
            out[f"mlp_out_dist_targ_{i}/kernel"], out[f"mlp_out_dist_targ_{i}/bias"] = m.kernel, m.bias
        out["distance_target/kernel"], out["distance_target/bias"] = self.distance_target.kernel, self.distance_target.bias
        return out

    def forward(self, e, target):
        if not e.is_cuda:
            raise RuntimeError("DistanceHead: no CPU path (distance_head_composed is the torch restatement)")
        return distance_head(e, target, self.params(), self.activation)
