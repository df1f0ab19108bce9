"""Fused pair operator for the large-head geometry (egt_pair_fwd / egt_pair_bwd in include/egt_amd.h):
(V_att, e') = norm_edge -> attention_gates / dense_edge_b -> EGT -> dense_edge_r + res_edge in ONE pair kernel per
direction (graph_xformer_model_base.py:195-218 around egt_layers.py:57-143).  The node-side layers of mha_block (norm_mha, dense_qkv,
dense_mha, the residual) run either as torch ops around it (`_PairOp`, route "torch") or inside the library's whole-block operator
(egt_pair_block_fwd / egt_pair_block_bwd: `_PairBlock`, route "library"); node_route() says which."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from .functional import _f32c, _u8c, _need_gpu
from .fused import _block_params, _desc, _lib_covers, _params_struct, _scratch, grad_sinks

# the eight edge-side parameters, in egt_block_params order (node-side slots stay NULL)
_EDGE = (("norm_edge", "gamma"), ("norm_edge", "beta"), ("attention_gates", "kernel"), ("attention_gates", "bias"),
         ("dense_edge_b", "kernel"), ("dense_edge_b", "bias"), ("dense_edge_r", "kernel"), ("dense_edge_r", "bias"))
_SLOTS = (0, 1, 2, 3, 4, 5, 12, 13)   # their positions in BLOCK_PARAM_FIELDS


def _struct(ts):
    full = [None] * len(L.BLOCK_PARAM_FIELDS)
    for s, t in zip(_SLOTS, ts):
        full[s] = t
    return _params_struct(full)


class _PairOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, e, key_mask, desc, *params):
        _need_gpu(qkv, e)
        lib = L.load()
        qkv = _f32c(qkv); e = _f32c(e)
        key_mask = _u8c(key_mask)
        ctx.param_objs = params
        params = tuple(_f32c(p) for p in params)
        B, N = e.shape[0], e.shape[1]
        Dh = qkv.shape[-1] // 3
        v_att = torch.empty(B, N, Dh, device=e.device, dtype=torch.float32)
        e_out = torch.empty_like(e)
        rowstats = torch.empty(B, N, desc.H, 4, device=e.device, dtype=torch.float32)
        desc.reserved = L.ATTN_WS_SHARED if any(ctx.needs_input_grad[:2]) or any(ctx.needs_input_grad[4:]) else 0
        ws = torch.empty(lib.egt_pair_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=e.device)
        L.check(lib.egt_pair_fwd(C.byref(desc), C.byref(_struct(params)), L.ptr(qkv), L.ptr(e), L.ptr(key_mask),
                                 L.ptr(v_att), L.ptr(e_out), L.ptr(rowstats), L.ptr(ws), L.current_stream()))
        ctx.desc = desc
        ctx.save_for_backward(qkv, e, key_mask, v_att, rowstats, ws if desc.reserved else None, *params)
        return v_att, e_out

    @staticmethod
    def backward(ctx, d_v_att, d_e_out):
        lib = L.load()
        qkv, e, key_mask, v_att, rowstats, ws, *params = ctx.saved_tensors
        desc = ctx.desc
        d_v_att = torch.zeros_like(v_att) if d_v_att is None else _f32c(d_v_att)
        d_e_out = torch.zeros_like(e) if d_e_out is None else _f32c(d_e_out)
        if ws is None:
            desc.reserved = 0
            ws = torch.empty(lib.egt_pair_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=e.device)
        d_qkv = torch.empty_like(qkv)
        d_e = torch.empty_like(e)
        bufs, rets = grad_sinks(ctx.param_objs)
        L.check(lib.egt_pair_bwd(C.byref(desc), C.byref(_struct(params)), L.ptr(qkv), L.ptr(e), L.ptr(key_mask),
                                 L.ptr(v_att), L.ptr(rowstats), L.ptr(d_v_att), L.ptr(d_e_out), L.ptr(d_qkv), L.ptr(d_e),
                                 C.byref(_struct(bufs)), L.ptr(ws), L.current_stream()))
        return (d_qkv, d_e, None, None) + tuple(rets)


class _PairBlock(torch.autograd.Function):
    """The whole block per C-ABI call (egt_pair_block_fwd / egt_pair_block_bwd): the node side on the library's MFMA GEMMs."""

    @staticmethod
    def forward(ctx, h, e, key_mask, desc, *params):
        _need_gpu(h, e)
        lib = L.load()
        h = _f32c(h); e = _f32c(e)
        key_mask = _u8c(key_mask)
        ctx.param_objs = params          # the Parameter objects themselves (grad_sinks looks at their .grad in the backward)
        params = tuple(_f32c(p) for p in params)
        h_out = torch.empty_like(h)
        e_out = torch.empty_like(e)
        saved = _scratch(lib.egt_pair_block_saved_bytes(C.byref(desc)), h.device)
        ws = _scratch(lib.egt_pair_block_workspace_bytes(C.byref(desc)), h.device)
        L.check(lib.egt_pair_block_fwd(C.byref(desc), C.byref(_params_struct(params)), L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                       L.ptr(h_out), L.ptr(e_out), L.ptr(saved), L.ptr(ws), L.current_stream()))
        ctx.desc = desc
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, e, key_mask, saved, *params)
        return h_out, e_out

    @staticmethod
    def backward(ctx, d_h_out, d_e_out):
        lib = L.load()
        h, e, key_mask, saved, *params = ctx.saved_tensors
        desc = ctx.desc
        d_h_out = torch.zeros_like(h) if d_h_out is None else _f32c(d_h_out)
        d_e_out = torch.zeros_like(e) if d_e_out is None else _f32c(d_e_out)
        d_h = torch.empty_like(h)
        d_e = torch.empty_like(e)
        bufs, rets = grad_sinks(ctx.param_objs)
        ws = _scratch(lib.egt_pair_block_workspace_bytes(C.byref(desc)), h.device)
        L.check(lib.egt_pair_block_bwd(C.byref(desc), C.byref(_params_struct(params)), L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                       L.ptr(saved), L.ptr(d_h_out), L.ptr(d_e_out), L.ptr(d_h), L.ptr(d_e),
                                       C.byref(_params_struct(bufs)), L.ptr(ws), L.current_stream()))
        return (d_h, d_e, None, None) + tuple(rets)


_PAIR_NODE = None


def node_route(blk, B, N) -> str:
    """Which node side block_pair takes when the caller does not force one: "library" (egt_pair_block_fwd / _bwd) where the
    process switch EGT_PAIR_NODE=1 is set (read once per process) and egt_pair_block_supported covers the block, else "torch"."""
    global _PAIR_NODE
    if _PAIR_NODE is None:
        _PAIR_NODE = os.environ.get("EGT_PAIR_NODE", "") not in ("", "0")
    return "library" if _PAIR_NODE and _lib_covers("egt_pair_block_supported", blk, B, N, torch.float32) else "torch"


def block_pair(blk, h, e, mask, node=None):
    """EGTBlock forward on the fused pair operator (fused.route decides when), mha_block (graph_xformer_model_base.py:106-145)
    inside edge_update_residual (:192-223).  `node`: "library" (the library's whole-block operator, node-side GEMMs included),
    "torch" (torch node-side Dense layers around the pair operator) or None (node_route() decides)."""
    B, N = h.shape[0], h.shape[1]
    m = blk.mha
    if node is None:
        node = node_route(blk, B, N)
    if node not in ("library", "torch"):
        raise ValueError(f"node must be 'library', 'torch' or None, got {node!r}")
    training = bool(blk.training and m.random_mask_prob > 0)
    seed = m.next_seed() if training else 0                 # the counter-hash stream of the fused / composed paths (oracle/rng_ref.py)
    desc = _desc(blk, B, N, training, seed)
    if node == "library":
        return _PairBlock.apply(h, e, mask, desc, *_block_params(blk, e))
    y = h                                                   # :107
    qkv = blk.dense_qkv(blk.norm_mha(h))                    # :109-113
    params = [getattr(getattr(blk, mod), attr) for mod, attr in _EDGE]
    v_att, e2 = _PairOp.apply(qkv, e, mask, desc, *params)  # :117-131, :195-218
    return blk.dense_mha(v_att) + y, e2                     # :136-140
