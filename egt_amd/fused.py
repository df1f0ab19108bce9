"""Fused attention block: one C-ABI call per layer per direction
(egt_block_fwd / egt_block_bwd in include/egt_amd.h)."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from .functional import _f32c, _u8c, _need_gpu

_GRAD_ORDER = (("norm_edge", "gamma"), ("norm_edge", "beta"),
               ("attention_gates", "kernel"), ("attention_gates", "bias"),
               ("dense_edge_b", "kernel"), ("dense_edge_b", "bias"),
               ("norm_mha", "gamma"), ("norm_mha", "beta"),
               ("dense_qkv", "kernel"), ("dense_qkv", "bias"),
               ("dense_mha", "kernel"), ("dense_mha", "bias"),
               ("dense_edge_r", "kernel"), ("dense_edge_r", "bias"))


_NO_STATIC_EDGE = None


def static_edge_disabled() -> bool:
    """EGT_NO_STATIC_EDGE=1 (read once per process): 'bias' stacks keep the per-layer route through the residual kernels."""
    global _NO_STATIC_EDGE
    if _NO_STATIC_EDGE is None:
        _NO_STATIC_EDGE = os.environ.get("EGT_NO_STATIC_EDGE", "") not in ("", "0")
    return _NO_STATIC_EDGE


_NO_SCALE_DEGREE = None


def scale_degree_disabled() -> bool:
    """EGT_NO_SCALE_DEGREE=1 (read once per process): blocks with degree scalers keep the composed route."""
    global _NO_SCALE_DEGREE
    if _NO_SCALE_DEGREE is None:
        _NO_SCALE_DEGREE = os.environ.get("EGT_NO_SCALE_DEGREE", "") not in ("", "0")
    return _NO_SCALE_DEGREE


def attn_dropout_fused(blk) -> bool:
    """The block asks for its attention dropout inside the fused pair kernels (EGTBlock(fused_attn_dropout=True), rate > 0)"""
    return bool(getattr(blk, "fused_attn_dropout", False)) and blk.mha.attn_dropout > 0


def _flags(blk, training=False, seed_device=False, static_edge=False, dropout=False) -> int:
    """egt_block_desc.flags of a block.  `dropout`: the call draws the attention-dropout mask in the kernels (training only:
    the library takes EGT_BF_ATTN_DROPOUT together with EGT_BF_TRAINING)"""
    flags = L.BF_STATIC_EDGE if static_edge else 0
    if dropout:
        flags |= L.BF_ATTN_DROPOUT | L.BF_TRAINING
    if seed_device:                  # egt_amd.graph.DeviceSeeds: the kernels complete the seed from HBM
        flags |= L.BF_SEED_DEVICE
    if blk.gated:
        flags |= L.BF_GATE
    if blk.edge_channel_type == "constrained":
        flags |= L.BF_ATTN_MASK
    if training:
        flags |= L.BF_TRAINING
    if blk.edge_channel_type == "bias":
        flags |= L.BF_NO_EDGE_LN
    if blk.mha.clip_logits_value is not None:
        flags |= L.BF_CLIP
    if blk.mha.scale_degree:         # degree scalers: the library answers for the flagged descriptor (fp32 edges, no static edge)
        flags |= L.BF_SCALE_DEGREE
        if blk.mha.scaler_type == "linear":
            flags |= L.BF_SCALER_LINEAR
    return flags


def _edge_code(edge_dtype) -> int:
    return L.EGT_BF16 if edge_dtype == torch.bfloat16 else L.EGT_F32


def _desc(blk, B, N, training, seed, edge_dtype=torch.float32, seed_device=None, static_edge=False, dropout=False) -> L.BlockDesc:
    lo = hi = 0.0
    if blk.mha.clip_logits_value is not None:
        lo, hi = float(blk.mha.clip_logits_value[0]), float(blk.mha.clip_logits_value[1])
    return L.BlockDesc(B=B, N=N, H=blk.num_heads, d=blk.model_width // blk.num_heads,
                       De=blk.edge_width, dtype=_edge_code(edge_dtype),
                       flags=_flags(blk, training, seed_device is not None, static_edge, dropout),
                       clip_lo=lo, clip_hi=hi,
                       random_mask_prob=float(blk.mha.random_mask_prob), ln_eps=1e-3,
                       reserved=L.rate_bits(blk.mha.attn_dropout) if dropout else 0,   # (the rate rides in `reserved`)
                       seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                       seed_device=None if seed_device is None else seed_device[0].ptr(seed_device[1]))


_LIB_ANSWERS = {}   # (entry point, B, N, H, d, De, dtype, flags, rate bits) -> bool


def _lib_covers(entry, blk, B, N, edge_dtype, static_edge=False, dropout=False) -> bool:
    """The library's answer (`entry`: egt_block_supported / egt_pair_supported) for a block's geometry, asked once per
    descriptor: the key is every descriptor field those read, built from the block's attributes as they are now.
    `dropout`: the question is about the descriptor flagged EGT_BF_ATTN_DROPOUT, with the block's rate."""
    key = (entry, B, N, blk.num_heads, blk.model_width // blk.num_heads, blk.edge_width, _edge_code(edge_dtype),
           _flags(blk, static_edge=static_edge, dropout=dropout), L.rate_bits(blk.mha.attn_dropout) if dropout else 0)
    ok = _LIB_ANSWERS.get(key)
    if ok is None:
        d = _desc(blk, B, N, False, 0, edge_dtype, static_edge=static_edge, dropout=dropout)
        ok = _LIB_ANSWERS[key] = bool(getattr(L.load(), entry)(C.byref(d)))
    return ok


def _unsupported(blk, training):
    """The tensor-independent conditions of the fused kernels: why they cannot run `blk` (None: they can, as far as the
    module's attributes go)."""
    if blk.edge_channel_type not in ("residual", "constrained", "bias"):
        return f"edge_channel_type {blk.edge_channel_type!r}"
    if blk.add_n_norm or blk.edge_activation is not None:
        return "add_n_norm / edge_activation"
    if blk.mha.scale_degree and blk.mha.num_virtual_nodes > 0:
        return "scale_degree with virtual nodes (the scaler of the virtual-node rows is not in the kernels)"
    if attn_dropout_fused(blk):          # the opt-in: the attribute itself is no reason any more
        if blk.mha.scale_degree:
            return "attn_dropout together with scale_degree (the two kernel instances are not combined)"
        if blk.mha.num_virtual_nodes > 0:
            return "scale_degree / attn_dropout / virtual nodes"
    elif blk.mha.attn_dropout > 0 or blk.mha.num_virtual_nodes > 0:
        return "scale_degree / attn_dropout / virtual nodes"
    if blk.mha.scale_degree and scale_degree_disabled():
        return "scale_degree (EGT_NO_SCALE_DEGREE is set)"
    if training and (blk.node_dropout > 0 or blk.edge_dropout > 0):
        return "node / edge dropout"
    if blk.model_width % blk.num_heads:
        return f"model_width {blk.model_width} is not a multiple of num_heads {blk.num_heads}"
    return None


_FLOATS = (torch.float32, torch.bfloat16)


def _covered(blk, B, N, node_dtype, edge_dtype, on_gpu, attn_mask, rand_mask, training):
    """What the fused kernels cover of one call: (edge route of the fused block or None, whether the fused pair operator
    covers it).  Every condition of either lives here and nowhere else."""
    if not on_gpu or _unsupported(blk, training) is not None:
        return None, False
    ect = blk.edge_channel_type
    edge_route = None
    drop = attn_dropout_fused(blk)       # training and evaluation both: the unflagged kernels run the evaluation
    if (node_dtype in _FLOATS and edge_dtype in _FLOATS and (ect != "constrained" or attn_mask)
            and _lib_covers("egt_block_supported", blk, B, N, edge_dtype)
            and (not drop or _lib_covers("egt_block_supported", blk, B, N, edge_dtype, dropout=True))):
        # static: the block was opted in by its EGTLayerStack (`_static_edge`), the process switch is off, the random mask is
        # the kernels' own, and the library covers the flagged descriptor
        static = (ect == "bias" and blk._static_edge and not rand_mask and not static_edge_disabled() and not drop
                  and _lib_covers("egt_block_supported", blk, B, N, edge_dtype, static_edge=True))
        edge_route = "static" if static else "per-layer-bias" if ect == "bias" else "chained-residual"
    # the pair operator (large heads): 'residual' edge channels, gated, fp32, no mask tensor of either kind
    pair = (ect == "residual" and blk.gated and not attn_mask and not rand_mask and not drop
            and node_dtype == torch.float32 and edge_dtype == torch.float32
            and _lib_covers("egt_pair_supported", blk, B, N, edge_dtype))
    return edge_route, pair


def route_core(blk, B, N, node_dtype, edge_dtype, on_gpu, attn_mask=False, rand_mask=False, keep=False, training=None):
    """Which route one call of `blk` takes, from plain values (`attn_mask`, `rand_mask`, `keep`: whether the call passes an
    attention mask, a random-mask tensor, injected dropout samples): (path, edge route) with path "fused" (edge route
    "static" | "per-layer-bias" | "chained-residual"), "fused-pair" or "composed" (edge route None).  fused=True / 'on'
    raises RuntimeError where neither fused route covers the configuration."""
    if blk.fused is False or blk.fused == "off":
        return "composed", None
    if getattr(blk, "attn_matmul", "f32") != "f32":
        return "composed", None     # bf16 attention products exist on the MFMA inner op only: neither fused route has the mode
    edge_route, pair = _covered(blk, B, N, node_dtype, edge_dtype, on_gpu, attn_mask, rand_mask,
                                blk.training if training is None else training)
    if edge_route is not None:
        return "fused", edge_route
    if pair and not keep:
        return "fused-pair", None
    if blk.fused in (True, "on") and not pair:
        raise RuntimeError("fused EGT block requested but this configuration is not covered by it")
    return "composed", None


def route(blk, h, e, attn_mask=None, rand_mask=None, node_keep=None, edge_keep=None):
    """route_core for the tensors of a call"""
    return route_core(blk, h.shape[0], h.shape[1], h.dtype, e.dtype, h.is_cuda and e.is_cuda, attn_mask is not None,
                      rand_mask is not None, node_keep is not None or edge_keep is not None)


def bf16_refusal(blk):
    """Why the fused block cannot run `blk` with bf16 edge tensors (None: it can).  bf16 edges exist only on the fused
    path -- the composed ops are fp32 -- so a bf16 model checks this at construction instead of failing at its first step:
    the tensor-independent conditions (in training mode: a model trains) and the library's answer for a bf16 descriptor
    (N does not change what the block covers)."""
    if blk.fused is False or blk.fused == 'off':
        return "the fused block is switched off"
    why = _unsupported(blk, True)
    if why is not None:
        return why
    if blk.mha.scale_degree:
        return "scale_degree with bf16 edge tensors (the degree-scaler kernels take fp32 edge tensors)"
    if _covered(blk, 1, 16, torch.float32, torch.bfloat16, True, True, False, True)[0] is None:
        return (f"geometry (num_heads {blk.num_heads}, head dim {blk.model_width // blk.num_heads}, "
                f"edge_width {blk.edge_width}) is not covered by the fused block")
    return None


def _edge_c(t, dtype=None):
    """edge tensor as the kernels take it: contiguous fp32 or bf16 (EGT_BF16: bf16 in HBM, fp32 math)"""
    if t is None:
        return None
    want = dtype if dtype is not None else (torch.bfloat16 if t.dtype == torch.bfloat16 else torch.float32)
    return t.to(want).contiguous()


def _node_io(h):
    """node tensors are fp32 at the C boundary; a bf16 caller gets its dtype back"""
    return (h.float(), h.dtype) if h.dtype != torch.float32 else (h, None)


def _params_struct(tensors) -> L.BlockParams:
    st = L.BlockParams()
    for name, t in zip(L.BLOCK_PARAM_FIELDS, tensors):
        setattr(st, name, None if t is None else t.data_ptr())
    return st


def grad_sinks(params):
    """Where a fused backward writes each parameter gradient, and what it returns to autograd.  A parameter whose .grad is a
    pre-bound view of a flat gradient buffer opened for direct writes (FlatGradAllReduce(direct=True)) receives its gradient
    IN that view and autograd gets None (no `grad += g` launch); everything else gets a fresh tensor as before."""
    bufs, rets = [], []
    for p in params:
        if p is None:
            bufs.append(None); rets.append(None)
            continue
        g = p.grad if getattr(p, "_egt_direct_grad", False) else None
        if g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape and g.device == p.device:
            bufs.append(g); rets.append(None)
        else:
            t = torch.empty_like(p, dtype=torch.float32)
            bufs.append(t); rets.append(t)
    return bufs, rets


def _call_tensors(h, e, key_mask, attn_mask, params):
    """the tensors of a block / stack call as the C-ABI takes them"""
    _need_gpu(h, e)
    attn_mask = None if attn_mask is None else _f32c(attn_mask.to(torch.float32))
    return _f32c(h), _edge_c(e), _u8c(key_mask), attn_mask, tuple(None if p is None else _f32c(p) for p in params)


def _scratch(nbytes, dev):
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _param_array(tensors, layers=1):
    """`layers` egt_block_params tables (parameters or gradient sinks), layer-major"""
    return (L.BlockParams * layers)(*[_params_struct(tensors[14 * i:14 * i + 14]) for i in range(layers)])


class _FusedBlock(torch.autograd.Function):
    """One block per C-ABI call (egt_block_fwd / egt_block_bwd).

    With EGT_BF_STATIC_EDGE in `desc` (a 'bias' block of an EGTLayerStack on the static-edge route; `first`: it is the stack's
    first layer) the second output IS the input e
    (an alias: no copy, no kernel write) and the next layer consumes it, so the per-layer chain of the edge gradient is
    kept: a layer receives the sum of all later layers' edge gradients as the gradient of that output, adds its own
    contribution and hands the result down.  One edge read per layer forward; one read + one read-modify-write per layer
    backward; no fills, no autograd adds.

    The accumulation is in place only in a buffer this class allocated itself (tagged `_egt_edge_acc` while it travels
    between the layers of a stack; the stack's first layer removes the tag before the gradient leaves).  A gradient tensor
    that came from anywhere else is read, and a fresh buffer is written: a caller's tensor is never mutated."""

    @staticmethod
    def forward(ctx, h, e, key_mask, attn_mask, rand_mask, desc, first, *params):
        lib = L.load()
        static = bool(desc.flags & L.BF_STATIC_EDGE)     # (block_fused passes no mask tensors then)
        ctx.param_objs = params          # the Parameter objects themselves (grad_sinks looks at their .grad in the backward)
        e_in = e
        h, e, key_mask, attn_mask, params = _call_tensors(h, e, key_mask, attn_mask, params)
        rand_mask = _u8c(rand_mask)
        dev = h.device
        h_out = torch.empty_like(h)
        e_out = None if static else torch.empty_like(e)
        saved = _scratch(lib.egt_block_saved_bytes(C.byref(desc)), dev)
        ws = _scratch(lib.egt_block_workspace_bytes(C.byref(desc)), dev)
        L.check(lib.egt_block_fwd(C.byref(desc), _param_array(params), L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                  L.ptr(attn_mask), L.ptr(rand_mask), L.ptr(h_out), L.ptr(e_out),
                                  L.ptr(saved), L.ptr(ws), L.current_stream()))
        ctx.desc, ctx.static, ctx.first = desc, static, first
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, e, key_mask, attn_mask, rand_mask, saved, *params)
        return h_out, (e_in if static else e_out)        # (returning an input: autograd hands out an alias of it)

    @staticmethod
    def backward(ctx, dh_out, de_out):
        lib = L.load()
        h, e, key_mask, attn_mask, rand_mask, saved, *params = ctx.saved_tensors
        desc = ctx.desc
        if dh_out is None:
            dh_out = torch.zeros_like(h)
        dh_out = _f32c(dh_out)
        own = (ctx.static and de_out is not None and getattr(de_out, "_egt_edge_acc", False) and de_out.dtype == e.dtype
               and de_out.is_contiguous() and de_out.shape == e.shape)
        if own:
            de = de_out                                 # ours: de[i] = de_out[i] + contribution, in place
        else:
            if de_out is None and not ctx.static:
                de_out = torch.zeros_like(e)            # 'bias': the caller continues with e itself
            if de_out is not None:                      # someone else's tensor: read only
                de_out = _edge_c(de_out, e.dtype)
            de = torch.empty_like(e)                    # (static, de_out None: the kernel takes NULL as zeros -- no fill)
        dh = torch.empty_like(h)
        grads, rets = grad_sinks(ctx.param_objs)
        ws = _scratch(lib.egt_block_workspace_bytes(C.byref(desc)), h.device)
        L.check(lib.egt_block_bwd(C.byref(desc), _param_array(params), L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                  L.ptr(attn_mask), L.ptr(rand_mask), L.ptr(saved), L.ptr(dh_out),
                                  L.ptr(de_out), L.ptr(dh), L.ptr(de), _param_array(grads), L.ptr(ws),
                                  L.current_stream()))
        if ctx.static:
            if not ctx.first:
                de._egt_edge_acc = True
            elif own:
                del de._egt_edge_acc                    # leaves the stack: an ordinary tensor from here on
        return (dh, de, None, None, None, None, None, *rets)


def _block_params(blk, e):
    """the 14 C-ABI parameters of a block.  'bias' edge channels (EGT-simple) have no norm_edge and no
    dense_edge_r: identity LN parameters and a zero update are passed instead (EGT_BF_NO_EDGE_LN)."""
    params = []
    mods = blk._modules                  # direct dict reads: nn.Module.__getattr__ was a quarter of the host time of a stack step
    for mod, attr in _GRAD_ORDER:
        m = mods.get(mod)
        params.append(None if m is None else m._parameters[attr])
    if blk.edge_channel_type == "bias":
        params[0], params[1] = blk._id_gamma, blk._id_beta       # constants owned by the block (no per-call allocation)
        params[12], params[13] = blk._zero_Wr, blk._zero_br
    return params


def block_fused(blk, h, e, mask, attn_mask, rand_mask=None, edge_route=None):
    """`edge_route`: route()'s answer for this call (asked here when the caller did not)"""
    if edge_route is None:
        edge_route = route(blk, h, e, attn_mask, rand_mask)[1]
    static = edge_route == "static"
    training = blk.training and blk.mha.random_mask_prob > 0.0
    # attention dropout in the kernels: in training mode only (evaluation runs the unflagged kernels).  Such a call always
    # consumes one seed -- also with an injected random mask or random_mask_prob == 0 -- as the composed operator does
    drop = blk.training and attn_dropout_fused(blk)
    draws = drop or (training and rand_mask is None)
    sdev = blk.mha.seed_device if draws else None
    seed = blk.mha.next_seed() if (draws and sdev is None) else 0
    desc = _desc(blk, h.shape[0], h.shape[1], training, seed, e.dtype, sdev, static_edge=static, dropout=drop)
    if static:
        # no identity / zero constants here: norm_edge and dense_edge_r do not exist for the kernels either
        mods = blk._modules
        params = [None if (mod in ("norm_edge", "dense_edge_r") or mods.get(mod) is None) else mods[mod]._parameters[attr]
                  for mod, attr in _GRAD_ORDER]
    else:
        params = _block_params(blk, e)
    if blk.edge_channel_type != "constrained":
        attn_mask = None
    blk.last_edge_route = edge_route
    h, hdt = _node_io(h)
    h2, e2 = _FusedBlock.apply(h, e, mask, attn_mask, rand_mask, desc, blk._static_first, *params)
    if blk.edge_channel_type == "bias" and not static:
        e2 = e                                         # :190 returns e0; the kernel's e' equals it (zero update)
    return (h2 if hdt is None else h2.to(hdt)), e2     # (static: e2 is autograd's alias of e, which chains the edge gradient)


# ------------------------------------------------------------------ layer stack ---
class _FusedStack(torch.autograd.Function):
    """All model_height attention blocks in one C-ABI call per direction
    (egt_stack_fwd / egt_stack_bwd)."""

    @staticmethod
    def forward(ctx, h, e, key_mask, attn_mask, desc, layers, holder, *params):
        lib = L.load()
        h, e, key_mask, attn_mask, params = _call_tensors(h, e, key_mask, attn_mask, params)
        dev = h.device
        h_out, e_out = torch.empty_like(h), torch.empty_like(e)
        saved = _scratch(lib.egt_stack_saved_bytes(C.byref(desc), layers), dev)
        ws = _scratch(lib.egt_stack_workspace_bytes(C.byref(desc), layers), dev)
        parr = _param_array(params, layers)
        L.check(lib.egt_stack_fwd(C.byref(desc), layers, parr, L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                  L.ptr(attn_mask), L.ptr(h_out), L.ptr(e_out), L.ptr(saved), L.ptr(ws),
                                  L.current_stream()))
        ctx.desc, ctx.layers, ctx.holder = desc, layers, holder
        ctx.parr = parr
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, e, key_mask, attn_mask, saved, *params)
        return h_out, e_out

    @staticmethod
    def backward(ctx, dh_out, de_out):
        lib = L.load()
        h, e, key_mask, attn_mask, saved, *params = ctx.saved_tensors
        desc, layers = ctx.desc, ctx.layers
        dev = h.device
        if de_out is None:
            de_out = torch.zeros_like(e)
        if dh_out is None:
            dh_out = torch.zeros_like(h)
        dh_out = _f32c(dh_out); de_out = _edge_c(de_out, e.dtype)
        dh, de = torch.empty_like(h), torch.empty_like(e)
        sink = getattr(ctx.holder, "sink", None) if ctx.holder is not None else None
        if sink is not None:
            # EGTStack.bind_flat_gradients(): every parameter's .grad already IS its view of the holder's persistent flat
            # buffer.  The C backward writes there (addresses by arithmetic: no per-parameter view, data_ptr() or
            # AccumulateGrad node — two thirds of the eager step's host time) and autograd gets nothing to accumulate.
            sizes = [p.numel() for p in params if p is not None]
            if sink.numel() != sum(sizes) or sink.device != dev:
                raise RuntimeError("bound flat gradient buffer does not match the stack's parameters; call bind_flat_gradients() again")
            base, off, ptrs = sink.data_ptr(), 0, []
            for p in params:
                if p is None:
                    ptrs.append(None)
                else:
                    ptrs.append(base + 4 * off)
                    off += p.numel()
            garr = C.cast((C.c_void_p * len(ptrs))(*ptrs), C.POINTER(L.BlockParams))
            # the parameters' .grad must still BE the views of the buffer: an optimizer.zero_grad() (set_to_none=True is torch's
            # default) between bind and backward would otherwise leave every stack parameter without a gradient, silently.
            # Checked on the first and last parameter only (the per-parameter walk is the host time this path exists to avoid)
            sp = getattr(ctx.holder, "sink_params", None)
            if sp:
                g0, g1 = sp[0].grad, sp[-1].grad
                if g0 is None or g1 is None or g0.data_ptr() != base or g1.data_ptr() != base + 4 * (off - sp[-1].numel()):
                    o2 = 0
                    for q in sp:
                        q.grad = sink[o2:o2 + q.numel()].view_as(q)
                        o2 += q.numel()
            ws = _scratch(lib.egt_stack_workspace_bytes(C.byref(desc), layers), dev)
            L.check(lib.egt_stack_bwd(C.byref(desc), layers, ctx.parr, L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                      L.ptr(attn_mask), L.ptr(saved), L.ptr(dh_out), L.ptr(de_out), L.ptr(dh),
                                      L.ptr(de), garr, L.ptr(ws), L.current_stream()))
            ctx.holder.flat = sink
            return (dh, de, None, None, None, None, None, *([None] * len(params)))
        # every parameter gradient is a view of ONE flat buffer: the data-parallel all-reduce
        # (egt_amd.dp) runs on it directly, and autograd adopts the views without copies
        sizes = [p.numel() for p in params if p is not None]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        pieces = iter(flat.split(sizes))          # one call for all views (the per-parameter slicing was ~0.4 ms of host time per step)
        grads = []
        for p in params:
            if p is None:
                grads.append(None)
            else:
                v = next(pieces)
                grads.append(v if p.dim() == 1 else v.view(p.shape))
        if ctx.holder is not None:
            ctx.holder.flat = flat
        ws = _scratch(lib.egt_stack_workspace_bytes(C.byref(desc), layers), dev)
        parr = ctx.parr                            # the forward's struct array: same parameter tensors (kept alive by saved_tensors)
        garr = _param_array(grads, layers)
        L.check(lib.egt_stack_bwd(C.byref(desc), layers, parr, L.ptr(h), L.ptr(e), L.ptr(key_mask),
                                  L.ptr(attn_mask), L.ptr(saved), L.ptr(dh_out), L.ptr(de_out), L.ptr(dh),
                                  L.ptr(de), garr, L.ptr(ws), L.current_stream()))
        return (dh, de, None, None, None, None, None, *grads)


def stack_supported(stack, h, e, attn_mask) -> bool:
    """one egt_stack_* call runs the stack: every block takes the fused route and they share one descriptor"""
    blocks = list(stack.blocks)
    if not blocks:
        return False
    b0 = blocks[0]
    for b in blocks:
        # (egt_stack_* carries no degree and draws no dropout: block by block)
        if route(b, h, e, attn_mask)[0] != "fused" or b.mha.scale_degree or attn_dropout_fused(b):
            return False
        same = (b.model_width == b0.model_width and b.edge_width == b0.edge_width and
                b.edge_channel_type == b0.edge_channel_type and b.gated == b0.gated and
                b.mha.clip_logits_value == b0.mha.clip_logits_value and
                b.mha.random_mask_prob == b0.mha.random_mask_prob and b.training == b0.training)
        if not same:
            return False
    return True


def stack_fused(stack, h, e, mask, attn_mask):
    blocks = list(stack.blocks)
    b0 = blocks[0]
    training = b0.training and b0.mha.random_mask_prob > 0.0
    sdev = b0.mha.seed_device if training else None
    seed = b0.mha.next_seed() if (training and sdev is None) else 0
    desc = _desc(b0, h.shape[0], h.shape[1], training, seed, e.dtype, sdev)
    params = []
    for blk in blocks:
        params += _block_params(blk, e)
    if b0.edge_channel_type != "constrained":
        attn_mask = None
    h, hdt = _node_io(h)
    h2, e2 = _FusedStack.apply(h, e, mask, attn_mask, desc, len(blocks), stack.grad_holder, *params)
    if b0.edge_channel_type == "bias":
        e2 = e
    return (h2 if hdt is None else h2.to(hdt)), e2


def layer_seed(seed: int, layer: int) -> int:
    """Seed of layer `layer` inside egt_stack_* (mirrors egt_block.hip:layer_seed)."""
    return (seed ^ (0x9E3779B97F4A7C15 * (layer + 1))) & 0xFFFFFFFFFFFFFFFF
