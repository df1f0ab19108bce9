"""ctypes binding of the C-ABI in include/egt_amd.h.

The library is loaded from egt_amd/lib/libegt_amd.so (built in-tree by
egt_amd/build.py).  There is NO fallback: if the HIP library is missing or a
call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EGT_AMD_LIB") or os.path.join(_HERE, "lib", "libegt_amd.so")   # EGT_AMD_LIB: A/B experiments with variant builds

# --- constants mirrored from include/egt_amd.h ---------------------------------
ABI_VERSION = 4   # include/egt_amd.h EGT_ABI_VERSION
EGT_OK = 0
EGT_E_NULL, EGT_E_SHAPE, EGT_E_DTYPE, EGT_E_FLAGS, EGT_E_HIP, EGT_E_WORKSPACE, EGT_E_RCCL = -1, -2, -3, -4, -5, -6, -7
EGT_F32 = 0
EGT_BF16 = 1   # fused block/stack, channel FFN, edge embedding: edge tensors bf16 in HBM, everything else fp32
F_EDGE_INPUT, F_GATE_INPUT, F_ATTN_MASK, F_SCALE_DEGREE = 0x001, 0x002, 0x004, 0x008
F_SCALER_LINEAR, F_TRAINING, F_CLIP = 0x010, 0x020, 0x040
ATTN_WS_SHARED = 0x1   # egt_attn_desc.reserved: one workspace for egt_attn_mfma_fwd and _bwd
ATTN_MM_BF16 = 0x2     # egt_attn_desc.reserved: bf16 operands / fp32 accumulate for the MFMA inner op's matrix products
EP_LAYERNORM, EP_GATES = 0x1, 0x2
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_ELU = 0, 1, 2, 3
# egt_block_desc.flags
BF_GATE, BF_ATTN_MASK, BF_TRAINING, BF_CLIP, BF_NO_EDGE_LN, BF_SEED_DEVICE = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
BF_STATIC_EDGE = 0x40   # 'bias' edge channels: e is an input only (with BF_NO_EDGE_LN; De = 8 pair kernels)
BF_SCALE_DEGREE, BF_SCALER_LINEAR = 0x80, 0x100   # degree scalers on the MFMA-tile pair kernels (fp32 edges, gated)
BF_ATTN_DROPOUT = 0x200   # attention dropout in the MFMA-tile pair kernels (training only); the rate: BlockDesc.reserved = rate_bits(rate)


def rate_bits(rate: float) -> int:
    """fp32 bit pattern of a dropout rate as the int32 that egt_block_desc.reserved carries under BF_ATTN_DROPOUT"""
    import struct
    return struct.unpack("<i", struct.pack("<f", float(rate)))[0]


class AttnDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("H", C.c_int32), ("d", C.c_int32),
                ("dtype", C.c_int32), ("flags", C.c_uint32),
                ("clip_lo", C.c_float), ("clip_hi", C.c_float),
                ("random_mask_prob", C.c_float), ("attn_dropout", C.c_float),
                ("num_virtual_nodes", C.c_int32), ("reserved", C.c_int32),
                ("seed", C.c_uint64)]


class EdgeDesc(C.Structure):
    _fields_ = [("rows", C.c_int64), ("De", C.c_int32), ("H", C.c_int32),
                ("dtype", C.c_int32), ("flags", C.c_uint32), ("act", C.c_int32),
                ("act_alpha", C.c_float), ("ln_eps", C.c_float), ("reserved", C.c_int32)]


class BlockDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("H", C.c_int32), ("d", C.c_int32),
                ("De", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_uint32),
                ("clip_lo", C.c_float), ("clip_hi", C.c_float),
                ("random_mask_prob", C.c_float), ("ln_eps", C.c_float),
                ("reserved", C.c_int32), ("seed", C.c_uint64), ("seed_device", C.c_void_p)]


class FfnDesc(C.Structure):
    _fields_ = [("rows", C.c_int64), ("width", C.c_int32), ("dtype", C.c_int32),
                ("activation", C.c_int32), ("ln_eps", C.c_float), ("matmul", C.c_int32), ("flags", C.c_int32)]


MM_F32, MM_BF16X3, MM_BF16 = 0, 1, 2   # egt_ffn_desc.matmul
FFN_WS_PREPARED = 1                      # egt_ffn_desc.flags


FFN_PARAM_FIELDS = ("norm_gamma", "norm_beta", "lr1_kernel", "lr1_bias", "lr2_kernel", "lr2_bias")


class FfnParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FFN_PARAM_FIELDS]


class XtalkDesc(C.Structure):   # egt_xtalk_desc; its parameter / gradient structs are FfnParams
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("De", C.c_int32), ("Dh", C.c_int32), ("s_e", C.c_int32),
                ("s_n", C.c_int32), ("dtype", C.c_int32), ("activation", C.c_int32), ("ln_eps", C.c_float),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


BLOCK_PARAM_FIELDS = (
    "norm_edge_gamma", "norm_edge_beta",
    "attention_gates_kernel", "attention_gates_bias",
    "dense_edge_b_kernel", "dense_edge_b_bias",
    "norm_mha_gamma", "norm_mha_beta",
    "dense_qkv_kernel", "dense_qkv_bias",
    "dense_mha_kernel", "dense_mha_bias",
    "dense_edge_r_kernel", "dense_edge_r_bias",
)


class BlockParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in BLOCK_PARAM_FIELDS]


class EmbedDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("De", C.c_int32), ("upto_hop", C.c_int32),
                ("clip_hops", C.c_int32), ("num_edge_features", C.c_int32), ("dtype", C.c_int32),
                ("num_float_features", C.c_int32), ("mask_value", C.c_float), ("reserved", C.c_int32)]


EH_LAYERNORM = 0x1   # egt_head_desc.flags


class HeadDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("De", C.c_int32), ("M0", C.c_int32), ("M1", C.c_int32),
                ("C", C.c_int32), ("dtype", C.c_int32), ("activation", C.c_int32), ("flags", C.c_int32),
                ("ln_eps", C.c_float), ("reserved", C.c_int32)]


HEAD_PARAM_FIELDS = ("edge_norm_final_gamma", "edge_norm_final_beta", "mlp_out_dist_targ_0_kernel",
                     "mlp_out_dist_targ_0_bias", "mlp_out_dist_targ_1_kernel", "mlp_out_dist_targ_1_bias",
                     "distance_target_kernel", "distance_target_bias")


class HeadParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in HEAD_PARAM_FIELDS]


NH_LAYERNORM = 0x1   # egt_node_head_desc.flags


class NodeHeadDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("W", C.c_int32), ("M0", C.c_int32), ("M1", C.c_int32),
                ("C", C.c_int32), ("activation", C.c_int32), ("flags", C.c_int32), ("ln_eps", C.c_float),
                ("reserved", C.c_int32)]


NODE_HEAD_PARAM_FIELDS = ("node_norm_final_gamma", "node_norm_final_beta", "mlp_out_0_kernel", "mlp_out_0_bias",
                          "mlp_out_1_kernel", "mlp_out_1_bias", "target_kernel", "target_bias")


class NodeHeadParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in NODE_HEAD_PARAM_FIELDS]


GH_LAYERNORM = 0x1            # egt_graph_head_desc.flags
GH_MAE, GH_XENT = 0, 1        # egt_graph_head_desc.loss


class GraphHeadDesc(C.Structure):   # (its parameter / gradient structs are NodeHeadParams)
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("W", C.c_int32), ("M0", C.c_int32), ("M1", C.c_int32),
                ("C", C.c_int32), ("nv", C.c_int32), ("loss", C.c_int32), ("activation", C.c_int32), ("flags", C.c_int32),
                ("ln_eps", C.c_float), ("reserved", C.c_int32)]


NE_INT, NE_FLOAT = 0, 1                       # egt_node_embed_desc.kind
NE_PE_NONE, NE_PE_SVD, NE_PE_EIG = 0, 1, 2    # egt_node_embed_desc.pe_kind
NE_TRANSFORM, NE_SIGNS = 0x1, 0x2             # egt_node_embed_desc.flags


class NodeEmbedDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("Dh", C.c_int32), ("nv", C.c_int32), ("kind", C.c_int32), ("R", C.c_int32),
                ("F", C.c_int32), ("pe_kind", C.c_int32), ("T", C.c_int32), ("sel", C.c_int32), ("flags", C.c_int32),
                ("mask_value", C.c_float), ("sign_stride", C.c_int32), ("reserved", C.c_int32)]


NODE_EMBED_PARAM_FIELDS = ("node_emb", "node_emb_bias", "pe_kernel", "pe_bias", "virtual_node_emb")


class NodeEmbedParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in NODE_EMBED_PARAM_FIELDS]


OPT_ADAM, OPT_RMSPROP, OPT_SGD = 0, 1, 2     # egt_optim_desc.algo
OPT_CLIP, OPT_ZERO_GRAD = 0x1, 0x2            # egt_optim_desc.flags
OPTIM_STATE_BYTES = 64                        # EGT_OPTIM_STATE_BYTES


class OptimDesc(C.Structure):
    _fields_ = [("algo", C.c_int32), ("flags", C.c_uint32), ("num_segments", C.c_int32), ("reserved", C.c_int32),
                ("total", C.c_int64), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("clip_value", C.c_float)]


class OptimSegment(C.Structure):
    _fields_ = [("param", C.c_void_p), ("offset", C.c_int64), ("count", C.c_int64)]


BATCH_NONE, BATCH_I32, BATCH_F32 = 0, 1, 2                     # egt_batch_desc.node_kind / edge_kind
BATCH_PE_NONE, BATCH_PE_SVD, BATCH_PE_EIGEN = 0, 1, 2           # egt_batch_desc.pe_kind
BATCH_TGT_GRAPH_F32, BATCH_TGT_GRAPH_I32, BATCH_TGT_NODE_I32 = 0, 1, 2   # egt_batch_desc.target_kind
BATCH_MARK_INVALID = 0x1                                        # egt_batch_desc.flags
BATCH_STORE_FIELDS = ("num_nodes", "node_off", "edge_off", "row_off", "edge_dst", "edge_feat", "node_rows", "pe_rows", "targets")
BATCH_OUT_FIELDS = ("graph_matrix", "feature_matrix", "node_features", "pe", "target", "num_nodes")


class BatchDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("records", C.c_int32), ("node_kind", C.c_int32), ("node_width", C.c_int32),
                ("edge_kind", C.c_int32), ("edge_width", C.c_int32), ("pe_kind", C.c_int32), ("pe_features", C.c_int32),
                ("target_kind", C.c_int32), ("flags", C.c_uint32), ("matrix_pad", C.c_float), ("mask_f", C.c_float),
                ("mask_i", C.c_int32), ("reserved", C.c_int32 * 2)]


class BatchStore(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in BATCH_STORE_FIELDS]


class BatchOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in BATCH_OUT_FIELDS]


class AccItem(C.Structure):     # egt_acc_item
    _fields_ = [("sum", C.c_void_p), ("count", C.c_void_p), ("count_value", C.c_float)]


ACC_MAX_ITEMS = 32              # egt_accumulate: 1 <= K <= 32


def params_struct(cls, fields, tensors):
    """A parameter struct of the C-ABI (`cls`, its `fields` in order) filled with the tensors' device pointers (None -> NULL)."""
    st = cls()
    for name, t in zip(fields, tensors):
        setattr(st, name, None if t is None else t.data_ptr())
    return st


class EGTLibraryError(RuntimeError):
    pass


_lib = None

_VP = C.c_void_p
_PROTOS = {
    "egt_last_error_string": (C.c_char_p, []),
    "egt_abi_version": (C.c_int, []),
    "egt_attn_fwd": (C.c_int, [C.POINTER(AttnDesc)] + [_VP] * 12),
    "egt_attn_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(AttnDesc)]),
    "egt_attn_bwd": (C.c_int, [C.POINTER(AttnDesc)] + [_VP] * 16),
    "egt_attn_mfma_supported": (C.c_int, [C.POINTER(AttnDesc), C.c_int]),
    "egt_attn_mfma_fwd_workspace_bytes": (C.c_size_t, [C.POINTER(AttnDesc)]),
    "egt_attn_mfma_workspace_bytes": (C.c_size_t, [C.POINTER(AttnDesc)]),
    "egt_attn_mfma_fwd": (C.c_int, [C.POINTER(AttnDesc)] + [_VP] * 11),
    "egt_attn_mfma_bwd": (C.c_int, [C.POINTER(AttnDesc)] + [_VP] * 15),
    "egt_mask_sample": (C.c_int, [C.c_int, C.c_uint64, C.c_float, C.c_int32, C.c_int32,
                                  C.c_int32, _VP, _VP]),
    "egt_seed_advance": (C.c_int, [_VP, C.c_int32, C.c_uint64, _VP]),
    "egt_edge_proj_fwd": (C.c_int, [C.POINTER(EdgeDesc)] + [_VP] * 10),
    "egt_edge_proj_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(EdgeDesc)]),
    "egt_edge_proj_bwd": (C.c_int, [C.POINTER(EdgeDesc)] + [_VP] * 17),
    "egt_edge_proj_bwd_acc": (C.c_int, [C.POINTER(EdgeDesc)] + [_VP] * 18),
    "egt_edge_update_fwd": (C.c_int, [C.POINTER(EdgeDesc)] + [_VP] * 6),
    "egt_edge_update_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(EdgeDesc)]),
    "egt_edge_update_bwd": (C.c_int, [C.POINTER(EdgeDesc)] + [_VP] * 8),
    "egt_node_mask_from_features": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    "egt_node_mask_from_float_features": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _VP, _VP]),
    "egt_constrained_edge_mask": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    "egt_edge_embed_supported": (C.c_int, [C.POINTER(EmbedDesc)]),
    "egt_edge_embed_hops_bytes": (C.c_size_t, [C.POINTER(EmbedDesc)]),
    "egt_edge_embed_workspace_bytes": (C.c_size_t, [C.POINTER(EmbedDesc)]),
    "egt_edge_embed_fwd": (C.c_int, [C.POINTER(EmbedDesc)] + [_VP] * 9),
    "egt_edge_embed_bwd": (C.c_int, [C.POINTER(EmbedDesc)] + [_VP] * 8),
    "egt_edge_embed_vn_supported": (C.c_int, [C.POINTER(EmbedDesc), C.c_int32]),
    "egt_edge_embed_vn_workspace_bytes": (C.c_size_t, [C.POINTER(EmbedDesc), C.c_int32]),
    "egt_edge_embed_vn_fwd": (C.c_int, [C.POINTER(EmbedDesc), C.c_int32] + [_VP] * 10),
    "egt_edge_embed_vn_bwd": (C.c_int, [C.POINTER(EmbedDesc), C.c_int32] + [_VP] * 9),
    "egt_distance_target": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    "egt_edge_head_supported": (C.c_int, [C.POINTER(HeadDesc)]),
    "egt_edge_head_workspace_bytes": (C.c_size_t, [C.POINTER(HeadDesc)]),
    "egt_edge_head_fwd": (C.c_int, [C.POINTER(HeadDesc), C.POINTER(HeadParams)] + [_VP] * 5),
    "egt_edge_head_bwd": (C.c_int, [C.POINTER(HeadDesc), C.POINTER(HeadParams)] + [_VP] * 4
                          + [C.POINTER(HeadParams)] + [_VP] * 2),
    "egt_node_head_supported": (C.c_int, [C.POINTER(NodeHeadDesc)]),
    "egt_node_head_workspace_bytes": (C.c_size_t, [C.POINTER(NodeHeadDesc)]),
    "egt_node_head_fwd": (C.c_int, [C.POINTER(NodeHeadDesc), C.POINTER(NodeHeadParams)] + [_VP] * 7),
    "egt_node_head_bwd": (C.c_int, [C.POINTER(NodeHeadDesc), C.POINTER(NodeHeadParams)] + [_VP] * 6
                          + [C.POINTER(NodeHeadParams)] + [_VP] * 2),
    "egt_graph_head_supported": (C.c_int, [C.POINTER(GraphHeadDesc)]),
    "egt_graph_head_workspace_bytes": (C.c_size_t, [C.POINTER(GraphHeadDesc)]),
    "egt_graph_head_fwd": (C.c_int, [C.POINTER(GraphHeadDesc), C.POINTER(NodeHeadParams)] + [_VP] * 7),
    "egt_graph_head_bwd": (C.c_int, [C.POINTER(GraphHeadDesc), C.POINTER(NodeHeadParams)] + [_VP] * 5
                           + [C.POINTER(NodeHeadParams)] + [_VP] * 2),
    "egt_node_embed_supported": (C.c_int, [C.POINTER(NodeEmbedDesc)]),
    "egt_node_embed_workspace_bytes": (C.c_size_t, [C.POINTER(NodeEmbedDesc)]),
    "egt_node_embed_fwd": (C.c_int, [C.POINTER(NodeEmbedDesc), C.POINTER(NodeEmbedParams)] + [_VP] * 6),
    "egt_node_embed_bwd": (C.c_int, [C.POINTER(NodeEmbedDesc)] + [_VP] * 4 + [C.POINTER(NodeEmbedParams)] + [_VP] * 2),
    "egt_dp_unique_id": (C.c_int, [_VP]),
    "egt_dp_init": (C.c_int, [_VP, C.c_int32, C.c_int32]),
    "egt_dp_allreduce": (C.c_int, [_VP, C.c_size_t, C.c_int32, _VP]),
    "egt_dp_world": (C.c_int, []),
    "egt_dp_rank": (C.c_int, []),
    "egt_dp_finalize": (C.c_int, []),
    "egt_prof_enable": (C.c_int, [C.c_int]),
    "egt_prof_filter": (C.c_int, [C.c_char_p]),
    "egt_prof_stride": (C.c_int, [C.c_int]),
    "egt_prof_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "egt_prof_names": (C.c_int, [C.c_char_p, C.c_size_t]),
    "egt_prof_collect_graph": (C.c_int, [C.c_int]),
    "egt_prof_forget_graphs": (C.c_int, []),
    "egt_block_supported": (C.c_int, [C.POINTER(BlockDesc)]),
    "egt_block_bwd_kernel": (C.c_char_p, [C.POINTER(BlockDesc)]),
    "egt_block_launch_form": (C.c_char_p, [C.POINTER(BlockDesc)]),
    "egt_block_plan_static": (C.c_int, [C.POINTER(BlockDesc)]),
    "egt_block_saved_bytes": (C.c_size_t, [C.POINTER(BlockDesc)]),
    "egt_block_workspace_bytes": (C.c_size_t, [C.POINTER(BlockDesc)]),
    "egt_block_fwd": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(BlockParams)] + [_VP] * 10),
    "egt_block_bwd": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(BlockParams)] + [_VP] * 10
                      + [C.POINTER(BlockParams)] + [_VP] * 2),
    "egt_stack_saved_bytes": (C.c_size_t, [C.POINTER(BlockDesc), C.c_int32]),
    "egt_stack_workspace_bytes": (C.c_size_t, [C.POINTER(BlockDesc), C.c_int32]),
    "egt_stack_tail_form": (C.c_char_p, [C.POINTER(BlockDesc), C.c_int32]),
    "egt_stack_fwd": (C.c_int, [C.POINTER(BlockDesc), C.c_int32, C.POINTER(BlockParams)] + [_VP] * 9),
    "egt_stack_bwd": (C.c_int, [C.POINTER(BlockDesc), C.c_int32, C.POINTER(BlockParams)] + [_VP] * 9
                      + [C.POINTER(BlockParams)] + [_VP] * 2),
    "egt_pair_supported": (C.c_int, [C.POINTER(BlockDesc)]),
    "egt_pair_workspace_bytes": (C.c_size_t, [C.POINTER(BlockDesc)]),
    "egt_pair_fwd": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(BlockParams)] + [_VP] * 8),
    "egt_pair_bwd": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(BlockParams)] + [_VP] * 9
                     + [C.POINTER(BlockParams)] + [_VP] * 2),
    "egt_pair_block_supported": (C.c_int, [C.POINTER(BlockDesc)]),
    "egt_pair_block_launch_form": (C.c_char_p, [C.POINTER(BlockDesc)]),
    "egt_pair_block_saved_bytes": (C.c_size_t, [C.POINTER(BlockDesc)]),
    "egt_pair_block_workspace_bytes": (C.c_size_t, [C.POINTER(BlockDesc)]),
    "egt_pair_block_fwd": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(BlockParams)] + [_VP] * 8),
    "egt_pair_block_bwd": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(BlockParams)] + [_VP] * 8
                           + [C.POINTER(BlockParams)] + [_VP] * 2),
    "egt_ffn_supported": (C.c_int, [C.POINTER(FfnDesc)]),
    "egt_ffn_workspace_bytes": (C.c_size_t, [C.POINTER(FfnDesc)]),
    "egt_ffn_fwd": (C.c_int, [C.POINTER(FfnDesc), C.POINTER(FfnParams)] + [_VP] * 4),
    "egt_ffn_bwd": (C.c_int, [C.POINTER(FfnDesc), C.POINTER(FfnParams)] + [_VP] * 3
                    + [C.POINTER(FfnParams)] + [_VP] * 2),
    "egt_xtalk_supported": (C.c_int, [C.POINTER(XtalkDesc)]),
    "egt_xtalk_workspace_bytes": (C.c_size_t, [C.POINTER(XtalkDesc)]),
    "egt_xtalk_launch_form": (C.c_char_p, [C.POINTER(XtalkDesc)]),
    "egt_xtalk_fwd": (C.c_int, [C.POINTER(XtalkDesc), C.POINTER(FfnParams)] + [_VP] * 8),
    "egt_xtalk_bwd": (C.c_int, [C.POINTER(XtalkDesc), C.POINTER(FfnParams)] + [_VP] * 9
                      + [C.POINTER(FfnParams)] + [_VP] * 2),
    "egt_optim_supported": (C.c_int, [C.POINTER(OptimDesc)]),
    "egt_optim_prepare": (C.c_int, [C.POINTER(OptimDesc), _VP, _VP]),
    "egt_optim_step": (C.c_int, [C.POINTER(OptimDesc)] + [_VP] * 6),
    "egt_batch_supported": (C.c_int, [C.POINTER(BatchDesc)]),
    "egt_batch_assemble": (C.c_int, [C.POINTER(BatchDesc), C.POINTER(BatchStore), _VP, C.POINTER(BatchOut), _VP]),
    "egt_batch_assemble_at": (C.c_int, [C.POINTER(BatchDesc), C.POINTER(BatchStore), _VP, _VP, C.POINTER(BatchOut), _VP]),
    "egt_accumulate": (C.c_int, [_VP, _VP, C.c_int32, _VP]),
}


def load():
    """Load (once) and return the ctypes library.  Raises EGTLibraryError when the
    HIP library has not been built — the product path never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EGTLibraryError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or python egt_amd/build.py)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.egt_abi_version() != ABI_VERSION:
        raise EGTLibraryError("ABI version mismatch")
    _lib = lib
    return lib


_EXC = {EGT_E_NULL: ValueError, EGT_E_SHAPE: AssertionError, EGT_E_DTYPE: TypeError,
        EGT_E_FLAGS: ValueError, EGT_E_HIP: RuntimeError, EGT_E_WORKSPACE: RuntimeError, EGT_E_RCCL: RuntimeError}


def check(rc: int):
    """Re-raise a C error code as the exception type the reference raises for the
    same condition (egt_layers.py:20-24 ValueError, :70 AssertionError)."""
    if rc == EGT_OK:
        return
    msg = load().egt_last_error_string().decode(errors="replace")
    raise _EXC.get(rc, RuntimeError)(f"egt_amd: {msg} (code {rc})")


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
