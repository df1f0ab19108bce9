"""The gradient-sink layout production makes: FlatGradAllReduce(direct=True) binds each parameter's .grad to the view of one
flat buffer at the running sum of numel(), and the fused backward writes through those views.  A view is aligned to its element
and to nothing more -- the C ABI's contract for gradient sinks (include/egt_amd.h, "Buffer contract") and what the U runs of
tests/test_memcontract_gpu.py and the whole-model test of tests/test_graph_gpu.py exercise.  This file pins the fact those rest
on: with the distance objective every scheme's model really hands over sinks that are off 16 bytes.  A reordering of the
parameters that makes the misaligned case disappear from the models fails here, not silently in the end-to-end tests."""
import pytest
import torch

from egt_amd import training as T
from egt_amd.dp import FlatGradAllReduce

DISTANCE = dict(distance_target=8, distance_loss=0.5)


def _bound(scheme, cfg):
    model = T.import_scheme(scheme)(dict(cfg)).get_model()
    params = model.trainable_parameters()
    fa = FlatGradAllReduce(params, direct=True)
    names = {id(p): n for n, p in model.named_parameters()}
    assert len(fa.params) == len(params) > 0
    return model, fa, [names[id(p)] for p in fa.params]


@pytest.mark.parametrize("cfg", [{}, DISTANCE], ids=["default", "distance"])
@pytest.mark.parametrize("scheme", T.SCHEMES)
def test_direct_sinks_are_the_contiguous_views_at_the_running_offset(scheme, cfg):
    model, fa, names = _bound(scheme, cfg)
    assert fa.flat.dtype == torch.float32 and fa.flat.data_ptr() % 16 == 0
    assert len(set(names)) == len(names)
    off, residues = 0, {}
    for p, n in zip(fa.params, names):
        g = p.grad
        assert g.is_contiguous() and g.shape == p.shape and g.dtype == torch.float32, n
        assert g.data_ptr() == fa.flat.data_ptr() + 4 * off, n          # the view at the running sum of numel(): no padding
        assert getattr(p, "_egt_direct_grad") is True                   # (what fused.grad_sinks hands to the kernels)
        residues[n] = off % 4
        off += p.numel()
    assert off == fa.flat.numel()
    dist = [n for n in names if n.startswith("dist_head.")]
    if not cfg:
        assert not dist
        return
    assert len(dist) == 8                                               # gamma, beta and three (kernel, bias) pairs
    bad = [n for n in dist if residues[n] == 0]
    assert not bad, f"{scheme}: 16-byte aligned distance-head sinks {bad}: the end-to-end tests no longer see a misaligned sink"


@pytest.mark.parametrize("scheme", ["cifar10.svd", "mnist.svd"])
def test_embedding_sinks_of_the_image_schemes_are_off_16_bytes_without_the_distance_objective(scheme):
    """node_emb.* and edge_emb.* follow a parameter of 4 k + 2 floats: misaligned in the default config too"""
    _, fa, names = _bound(scheme, {})
    emb = [p for p, n in zip(fa.params, names) if n.startswith(("node_emb.", "edge_emb."))]
    assert emb and all((p.grad.data_ptr() - fa.flat.data_ptr()) % 16 for p in emb)
