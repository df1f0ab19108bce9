"""egt_amd — MI355X-native EGT edge-augmented attention hot path.

Public surface (mirrors the reference's operator interface for this path):
    EGT, EGTBlock, EGTStack, custom_layers      (egt_amd.layers)
    egt_attention, edge_proj, edge_update        (egt_amd.functional)
    FlatGradAllReduce, shard_batch               (egt_amd.dp)
    FFN, ffn                                     (egt_amd.ffn: the ffn_block step after the attention block)
    node_mask_from_features, node_mask_from_masking, constrained_edge_mask   (egt_amd.masks: mask producers)
    distance_target, DistanceHead                (egt_amd.head: the distance objective of the *_spe_do configs)
    node_head_loss, node_head_composed           (egt_amd.node_head: readout + class-weighted loss of PATTERN / CLUSTER)
    graph_head_loss, graph_head_composed         (egt_amd.graph_head: graph-level readout + loss of ZINC / CIFAR10 / MNIST)
    node_embed.node_embed, node_embed_composed   (egt_amd.node_embed: node features -> the stack's h and mask, every model)
    xtalk_ffn, xtalk_ffn_composed                (egt_amd.xtalk: the FFN pair of a layer with node<->edge cross-talk, fused edge side / torch ops)
    FlatOptimizer, plan_items                    (egt_amd.optim: Adam / RMSprop / SGD as two launches over the flat gradient buffer)
    DeviceSeeds, GraphedStep                     (egt_amd.graph: hipGraph capture of a step, device-resident mask seeds)
"""
from .layers import EGT, EGTBlock, EGTStack, EGTLayerStack, custom_layers, KerasDense, KerasLayerNorm  # noqa: F401
from .functional import AttnConfig, egt_attention, edge_proj, edge_update, mask_sample  # noqa: F401
from .ffn import FFN, ffn  # noqa: F401
from .xtalk import xtalk_ffn, xtalk_ffn_composed, xtalk_supported  # noqa: F401
from .model import (ZincDCTransformer, PatternDCTransformer, Cifar10DCTransformer, ClusterDCTransformer, MnistDCTransformer, sparse_xent_loss, edge_embed, mae_loss, weighted_sparse_xent_loss,  # noqa: F401
                    class_weights_from_sizes)
from .head import distance_target, DistanceHead, distance_head, distance_head_composed  # noqa: F401
from .node_head import node_head_loss, node_head_composed, node_head_supported  # noqa: F401
from .graph_head import graph_head_loss, graph_head_composed, graph_head_supported  # noqa: F401
from .node_embed import node_embed_composed, node_embed_supported  # noqa: F401  (node_embed itself stays in its module: the name is the module's)
from .graph import DeviceSeeds, GraphedStep  # noqa: F401
from .optim import FlatOptimizer, plan_items, flat_to_state, state_to_flat  # noqa: F401
from .masks import node_mask_from_features, node_mask_from_masking, constrained_edge_mask  # noqa: F401

__all__ = ["EGT", "EGTBlock", "EGTStack", "EGTLayerStack", "custom_layers", "AttnConfig", "egt_attention",
           "edge_proj", "edge_update", "mask_sample", "FFN", "ffn", "xtalk_ffn", "xtalk_ffn_composed", "xtalk_supported", "node_mask_from_features",
           "node_mask_from_masking", "constrained_edge_mask", "ZincDCTransformer", "PatternDCTransformer", "Cifar10DCTransformer", "ClusterDCTransformer", "MnistDCTransformer", "sparse_xent_loss", "edge_embed", "mae_loss",
           "weighted_sparse_xent_loss", "class_weights_from_sizes", "DeviceSeeds", "GraphedStep",
           "distance_target", "DistanceHead", "distance_head", "distance_head_composed",
           "node_head_loss", "node_head_composed", "node_head_supported",
           "graph_head_loss", "graph_head_composed", "graph_head_supported",
           "node_embed_composed", "node_embed_supported",
           "FlatOptimizer", "plan_items", "flat_to_state", "state_to_flat"]
