"""Channel FFN with node<->edge cross-talk (node2edge_xtalk / edge2node_xtalk of the reference's transform_embeddings,
lib/models/graph_xformer_model_base.py:227-324).  Per layer, with xn = fnn_lr1_node(LN(h)) [B,N,Hn] and
xe = fnn_lr1_edge(LN(e)) [B,N,N,He], both WITHOUT activation:

    edge -> node (fraction a > 0):  xe = [er | ec | tail], widths s_e, s_e, He - 2 s_e, s_e = round(a He / mult)
        hn = divide_no_nan(sum_i m_i er[:, i] + sum_j m_j ec[:, :, j], sum m)             [B,N,s_e]
    node -> edge (fraction b > 0):  xn = [hr | hc | tail], widths s_n, s_n, Hn - 2 s_n, s_n = round(b Hn / mult)
        en[b,i,j] = hr[b,i] + hc[b,j]                                                       [B,N,N,s_n]
    h' = h + fnn_lr2_node(act([xn tail | hn])),   e' = e + fnn_lr2_edge(act([xe tail | en]))

`xtalk_ffn` runs the edge side in the fused kernels of csrc/egt_xtalk.hip (egt_xtalk_fwd / egt_xtalk_bwd: the [B,N,N,He] hidden
tensor and the broadcast never reach HBM) and the three small node-side operations as torch ops; `xtalk_ffn_composed` is the same
result from torch ops alone, for the geometries the library declines.  The fused op has no CPU path."""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from .functional import _f32c, _need_gpu

_ACT = {"relu": L.ACT_RELU, "elu": L.ACT_ELU}
LN_EPS = 1e-3


def split_widths(edge_width, model_width, node2edge, edge2node, ffn_multiplier=2.0):
    """(s_e, s_n): the channels each side hands over (the reference's nx_s, graph_xformer_model_base.py:270, :286)"""
    he, hn = round(edge_width * ffn_multiplier), round(model_width * ffn_multiplier)
    s_e = round(edge2node * he / ffn_multiplier) if edge2node > 0 else 0
    s_n = round(node2edge * hn / ffn_multiplier) if node2edge > 0 else 0
    if 2 * s_e > he or 2 * s_n > hn:
        raise ValueError(f"cross-talk fractions take more than the hidden channels: 2*{s_e} of {he} edge, 2*{s_n} of {hn} node")
    return s_e, s_n


def lr2_widths(edge_width, model_width, node2edge, edge2node, ffn_multiplier=2.0):
    """(node, edge) input widths of fnn_lr2_node / fnn_lr2_edge after the exchange"""
    s_e, s_n = split_widths(edge_width, model_width, node2edge, edge2node, ffn_multiplier)
    return round(model_width * ffn_multiplier) - 2 * s_n + s_e, round(edge_width * ffn_multiplier) - 2 * s_e + s_n


def _desc(B, N, De, Dh, s_e, s_n, activation, eps=LN_EPS, dtype=torch.float32) -> L.XtalkDesc:
    if activation not in _ACT:
        raise ValueError(f"cross-talk FFN activation must be one of {sorted(_ACT)} (got {activation!r})")
    return L.XtalkDesc(B=B, N=N, De=De, Dh=Dh, s_e=s_e, s_n=s_n, dtype=L.EGT_F32 if dtype == torch.float32 else L.EGT_BF16,
                       activation=_ACT[activation], ln_eps=eps, flags=0, reserved=0)


def xtalk_supported(B, N, De, Dh, s_e, s_n, activation="elu", dtype=torch.float32) -> bool:
    """whether the fused kernels cover the geometry: the library's answer (egt_xtalk_supported)"""
    return activation in _ACT and bool(L.load().egt_xtalk_supported(C.byref(_desc(B, N, De, Dh, s_e, s_n, activation, dtype=dtype))))


def _act(x, activation):
    return F.elu(x) if activation == "elu" else torch.relu(x)


def _dense(x, kernel, bias):
    if x.is_cuda and x.dtype == kernel.dtype:
        return torch.addmm(bias, x.reshape(-1, x.shape[-1]), kernel).view(*x.shape[:-1], kernel.shape[1])
    return x @ kernel + bias


def xtalk_ffn_composed(h, e, mask, node_params, edge_params, node2edge=0.0, edge2node=0.0, activation="elu", eps=LN_EPS):
    """(h', e') from torch ops: the reference's ffn_block with cross-talk, statement by statement.  *_params: (norm gamma,
    norm beta, lr1 kernel, lr1 bias, lr2 kernel, lr2 bias), Keras layouts."""
    gn, bn, w1n, b1n, w2n, b2n = node_params
    ge, be, w1e, b1e, w2e, b2e = edge_params
    s_e, s_n = split_widths(e.shape[-1], h.shape[-1], node2edge, edge2node)
    xn = _dense(F.layer_norm(h, (h.shape[-1],), gn, bn, eps), w1n, b1n)
    xe = _dense(F.layer_norm(e, (e.shape[-1],), ge, be, eps), w1e, b1e)
    hn = en = None
    if s_e:
        m = mask.to(h.dtype)
        er, ec, xe = torch.split(xe, [s_e, s_e, xe.shape[-1] - 2 * s_e], dim=3)
        tot = (er * m[:, :, None, None]).sum(dim=1) + (ec * m[:, None, :, None]).sum(dim=2)
        cnt = m.sum(dim=1)[:, None, None]
        hn = torch.where(cnt != 0, tot / torch.where(cnt != 0, cnt, torch.ones_like(cnt)), torch.zeros_like(tot))   # divide_no_nan
    if s_n:
        hr, hc, xn = torch.split(xn, [s_n, s_n, xn.shape[-1] - 2 * s_n], dim=2)
        en = hr[:, :, None, :] + hc[:, None, :, :]
    if hn is not None:
        xn = torch.cat([xn, hn], dim=-1)
    if en is not None:
        xe = torch.cat([xe, en], dim=-1)
    return h + _dense(_act(xn, activation), w2n, b2n), e + _dense(_act(xe, activation), w2e, b2e)


def _pstruct(tensors) -> L.FfnParams:
    return L.params_struct(L.FfnParams, L.FFN_PARAM_FIELDS, tensors)


class _XtalkEdge(torch.autograd.Function):
    """(e, mask, hr, hc) -> (e', hn) on egt_xtalk_fwd / egt_xtalk_bwd; hr / hc are None with s_n = 0, hn is [B,N,0] with s_e = 0"""

    @staticmethod
    def forward(ctx, e, mask, hr, hc, desc, *params):
        _need_gpu(e)
        lib = L.load()
        e, mask = _f32c(e), _f32c(mask)
        hr, hc = _f32c(hr), _f32c(hc)
        ctx.param_objs = params
        params = tuple(_f32c(p) for p in params)
        e_out = torch.empty_like(e)
        hn = torch.empty(desc.B, desc.N, desc.s_e, dtype=torch.float32, device=e.device)
        ws = torch.empty(lib.egt_xtalk_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=e.device)
        pst = _pstruct(params)
        L.check(lib.egt_xtalk_fwd(C.byref(desc), C.byref(pst), L.ptr(e), L.ptr(mask), L.ptr(hr), L.ptr(hc), L.ptr(e_out),
                                  L.ptr(hn) if desc.s_e else None, L.ptr(ws), L.current_stream()))
        ctx.desc, ctx.has_n = desc, hr is not None
        ctx.save_for_backward(e, mask, *((hr, hc) if hr is not None else ()), *params)
        return e_out, hn

    @staticmethod
    def backward(ctx, d_e_out, d_hn):
        lib = L.load()
        desc = ctx.desc
        e, mask, *rest = ctx.saved_tensors
        hr, hc = (rest[0], rest[1]) if ctx.has_n else (None, None)
        params = rest[2:] if ctx.has_n else rest
        d_e_out = _f32c(d_e_out)
        d_hn = _f32c(d_hn) if desc.s_e else None
        d_e = torch.empty_like(e)
        d_hr = torch.empty_like(hr) if ctx.has_n else None
        d_hc = torch.empty_like(hc) if ctx.has_n else None
        from .fused import grad_sinks
        grads, rets = grad_sinks(ctx.param_objs)
        ws = torch.empty(lib.egt_xtalk_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=e.device)
        pst, gst = _pstruct(params), _pstruct(grads)
        L.check(lib.egt_xtalk_bwd(C.byref(desc), C.byref(pst), L.ptr(e), L.ptr(mask), L.ptr(hr), L.ptr(hc), L.ptr(d_e_out),
                                  L.ptr(d_hn), L.ptr(d_e), L.ptr(d_hr), L.ptr(d_hc), C.byref(gst), L.ptr(ws), L.current_stream()))
        return (d_e, None, d_hr, d_hc, None, *rets)


def xtalk_ffn(h, e, mask, node_params, edge_params, node2edge=0.0, edge2node=0.0, activation="elu", eps=LN_EPS):
    """(h', e'): the edge side in the fused kernels, the node side (lr1 Dense, concat, lr2 Dense on [B,N,.]) as torch ops.
    Raises ValueError for a geometry the library declines (`xtalk_ffn_composed` covers those)."""
    _need_gpu(h, e)
    gn, bn, w1n, b1n, w2n, b2n = node_params
    B, N, Dh = h.shape
    De = e.shape[-1]
    s_e, s_n = split_widths(De, Dh, node2edge, edge2node)
    desc = _desc(B, N, De, Dh, s_e, s_n, activation, eps, e.dtype)
    if tuple(e.shape) != (B, N, N, De) or not L.load().egt_xtalk_supported(C.byref(desc)):
        raise ValueError(f"fused cross-talk FFN covers fp32, De 16/32/64, Dh 48/64, exchanged widths that are multiples of 4; got "
                         f"e {tuple(e.shape)} {e.dtype}, h {tuple(h.shape)}, s_e {s_e}, s_n {s_n}")
    xn = _dense(F.layer_norm(h, (Dh,), gn, bn, eps), w1n, b1n)
    hr = hc = None
    if s_n:
        hr, hc, xn = torch.split(xn, [s_n, s_n, xn.shape[-1] - 2 * s_n], dim=2)
        hr, hc = hr.contiguous(), hc.contiguous()
    e_out, hn = _XtalkEdge.apply(e, mask.to(torch.float32), hr, hc, desc, *edge_params)
    if s_e:
        xn = torch.cat([xn, hn], dim=-1)
    return h + _dense(_act(xn, activation), w2n, b2n), e_out


def xtalk_node_only(h, node_params, s_n, activation="elu", eps=LN_EPS):
    """h' of a cross-talk layer whose edge output nobody reads and that receives nothing from the edges (edge2node_xtalk = 0):
    fnn_lr1_node, the hr / hc channels dropped, activation, fnn_lr2_node, residual -- the edge side is not run"""
    gn, bn, w1n, b1n, w2n, b2n = node_params
    xn = _dense(F.layer_norm(h, (h.shape[-1],), gn, bn, eps), w1n, b1n)
    return h + _dense(_act(xn[..., 2 * s_n:], activation), w2n, b2n)


class XtalkFFNParams(nn.Module):
    """The parameters of one channel type's FFN in a cross-talk layer, under the attribute and Keras names of egt_amd.ffn.FFN
    (norm_fnn_<tag>, fnn_lr1_<tag>, fnn_lr2_<tag>); fnn_lr2 takes `lr2_in` channels, the width after the exchange."""

    def __init__(self, width: int, lr2_in: int, ffn_multiplier: float = 2.0):
        super().__init__()
        hid = round(width * ffn_multiplier)
        self.width = width
        self.norm_gamma = nn.Parameter(torch.ones(width))
        self.norm_beta = nn.Parameter(torch.zeros(width))
        lim1, lim2 = math.sqrt(6.0 / (width + hid)), math.sqrt(6.0 / (lr2_in + width))   # Keras Dense default: glorot_uniform
        self.lr1_kernel = nn.Parameter(torch.empty(width, hid).uniform_(-lim1, lim1))
        self.lr1_bias = nn.Parameter(torch.zeros(hid))
        self.lr2_kernel = nn.Parameter(torch.empty(lr2_in, width).uniform_(-lim2, lim2))
        self.lr2_bias = nn.Parameter(torch.zeros(width))

    def tensors(self):
        return (self.norm_gamma, self.norm_beta, self.lr1_kernel, self.lr1_bias, self.lr2_kernel, self.lr2_bias)

    def keras_named_parameters(self, tag: str):
        return {f"norm_fnn_{tag}/gamma": self.norm_gamma, f"norm_fnn_{tag}/beta": self.norm_beta,
                f"fnn_lr1_{tag}/kernel": self.lr1_kernel, f"fnn_lr1_{tag}/bias": self.lr1_bias,
                f"fnn_lr2_{tag}/kernel": self.lr2_kernel, f"fnn_lr2_{tag}/bias": self.lr2_bias}
