"""Device-resident datasets on the GPU (egt_amd/device_data.py, csrc/egt_batch.hip): every batch DeviceGraphDataset yields is
the host pipeline's batch for the same seed -- same keys, dtypes, shapes and bits -- and a scheme trained from it reproduces
the run trained from the host pipeline.  The stores are synthetic (tests/device_data_cases.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import device_data_cases as DC
from egt_amd import data as D

pytestmark = pytest.mark.gpu
CASES = [(name, level) for name, levels in DC.LEVELS.items() for level in levels]
FIXED = {"zinc": 40, "zinc_full": 40, "cifar10": 150}          # the specs' own max_length


def _pair(path, name, level, gpu, seed=3, exclude=(), **kw):
    """(host dataset, device dataset) over the same store with the same seed"""
    kw = dict(dict(level=level, max_length=None, max_shuffle_len=6, seed=seed, prefetch_batch=False, num_features=4), **kw)
    if level == "svd":
        kw.setdefault("return_mat", True)
    host, other = D.GraphDataset(name, path, **kw), D.GraphDataset(name, path, **kw)
    host.exclude(exclude); other.exclude(exclude)
    return host, other.to_device(gpu)


def _same(hb, db, gpu, where):
    assert list(hb) == list(db), (where, list(hb), list(db))
    for k, hv in hb.items():
        dv = db[k]
        if not torch.is_tensor(hv):
            assert hv == dv, (where, k)
            continue
        assert dv.device.type == "cuda" and dv.dtype == hv.dtype and dv.shape == hv.shape, (where, k, dv.dtype, dv.shape, hv.dtype, hv.shape)
        assert torch.equal(dv, hv.to(gpu)), (where, k)


def _compare_epochs(host, dev, gpu, batch_size, epochs=2, **kw):
    h_sets, d_sets = host.get_batched_data(batch_size, **kw), dev.get_batched_data(batch_size, **kw)
    total = 0
    for si, (hs, dset) in enumerate(zip(h_sets, d_sets)):
        assert len(hs) == len(dset)
        for ep in range(epochs):
            hbs, dbs = list(hs), list(dset)
            assert len(hbs) == len(dbs), (si, ep, len(hbs), len(dbs))
            for i, (hb, db) in enumerate(zip(hbs, dbs)):
                _same(hb, db, gpu, (si, ep, i))
            total += len(hbs)
    return total


@pytest.mark.parametrize("name,level", CASES)
def test_batches_equal_the_host_pipeline(name, level, tmp_path, gpu, egt_lib):
    path = DC.edge_case_store(tmp_path, name)
    host, dev = _pair(path, name, level, gpu)
    assert dev.nbytes > 0
    assert _compare_epochs(host, dev, gpu, 4) == 2 * (4 + 2)              # 13 graphs: the last training batch has one graph
    keys = set(next(iter(dev.get_batched_data(4)[0])))
    pe = {"svd": {"singular_vectors"}, "eigen": {"eigen_vectors"}}.get(level, set())
    assert keys == {"num_nodes", "node_features", "target", "graph_matrix"} | pe | ({"feature_matrix"} if D.SPECS[name].fm_tail is not None else set())
    if name in FIXED:                                                     # a fixed padded length
        host, dev = _pair(path, name, level, gpu, max_length=FIXED[name])
        _compare_epochs(host, dev, gpu, 4, epochs=1)
        assert next(iter(dev.get_batched_data(4)[0]))["graph_matrix"].shape == (4, FIXED[name], FIXED[name])


@pytest.mark.parametrize("name,level", [("zinc", "svd"), ("sbm_pattern", "eigen"), ("cifar10", "svd")])
def test_exclude_remainder_shards_and_map_fn(name, level, tmp_path, gpu, egt_lib):
    path = DC.edge_case_store(tmp_path, name)
    excl = ["record_name", "num_nodes", {"svd": "singular_vectors", "eigen": "eigen_vectors"}[level]]
    host, dev = _pair(path, name, level, gpu, exclude=excl)
    _compare_epochs(host, dev, gpu, 4)
    b = next(iter(dev.get_batched_data(4)[0]))
    assert not set(excl) & set(b) and "graph_matrix" in b
    host, dev = _pair(path, name, level, gpu)
    assert _compare_epochs(host, dev, gpu, 4, drop_remainder=True) == 2 * (3 + 1)
    # 13 training graphs in batches of 4 over 2 ranks: the one-graph last batch is dropped by both ranks of a training pass;
    # 5 validation graphs: rank 0 takes the one graph of the short batch and rank 1 skips it
    for rank, n_val in ((0, 2), (1, 1)):
        host, dev = _pair(path, name, level, gpu)
        tr, va = dev.get_batched_data(4, shard=(rank, 2))
        bs = list(tr)
        assert len(bs) == 3 and all(b["_local_count"] == 2 and b["_global_count"] == 4 and len(b["target"]) == 2 for b in bs)
        assert len(list(va)) == n_val
        host, dev = _pair(path, name, level, gpu)
        assert _compare_epochs(host, dev, gpu, 4, shard=(rank, 2)) == 2 * (3 + n_val)
    host, dev = _pair(path, name, level, gpu)
    fn = D.CreateTargets("target")
    hs, dset = host.get_batched_data(4, map_fns=fn)[0], dev.get_batched_data(4, map_fns=fn)[0]
    for (hx, hy), (dx, dy) in zip(hs, dset):
        _same(hx, dx, gpu, "X"); _same(hy, dy, gpu, "Y")
        assert set(dy) == {"target"}


def _largest_supported(lib):
    from egt_amd import _lib as L
    from egt_amd.device_data import MAX_NODES
    mk = lambda N: L.BatchDesc(B=3, N=N, records=3, node_kind=L.BATCH_F32, node_width=5, edge_kind=L.BATCH_F32, edge_width=1,
                               target_kind=L.BATCH_TGT_GRAPH_I32, flags=L.BATCH_MARK_INVALID, mask_f=-1.0, mask_i=-1)
    assert lib.egt_batch_supported(C.byref(mk(MAX_NODES))) == 1 and lib.egt_batch_supported(C.byref(mk(MAX_NODES + 1))) == 0
    return MAX_NODES


@pytest.mark.parametrize("name,which", [("cifar10", 190), ("sbm_pattern", 187), ("cifar10", "largest")])
def test_large_graphs(name, which, tmp_path, gpu, egt_lib):
    """row tiles that do not divide N (190 = 5 x 32 + 30, 512 = 34 x 15 + 2) and, at N = 187, spans that start off a 16-byte
    boundary (187 x 187 is odd)"""
    big = _largest_supported(egt_lib) if which == "largest" else which
    recs = DC.big_records(name, (big // 2 + 1, big, 3))
    path = DC.write_store(tmp_path, name, recs, recs[:2], f"_{big}")
    host, dev = _pair(path, name, "matrix", gpu)
    _compare_epochs(host, dev, gpu, 3, epochs=1)
    b = next(iter(dev.get_batched_data(3)[0]))
    assert b["graph_matrix"].shape == (3, big, big)
    if which == "largest":      # one node more has no kernel: an error, not a host fallback
        recs = DC.big_records(name, (big + 1, 5))
        dev = D.GraphDataset(name, DC.write_store(tmp_path, name, recs, recs, "_over"), level="matrix", max_length=None).to_device(gpu)
        with pytest.raises(ValueError, match="does not cover"):
            next(iter(dev.get_batched_data(2)[0]))
    too_small = D.GraphDataset(name, path, level="matrix", max_length=big - 1).to_device(gpu)
    with pytest.raises(ValueError, match="exceeds"):
        next(iter(too_small.get_batched_data(3)[0]))


@pytest.mark.parametrize("name,level", [("zinc", "svd"), ("cifar10", "svd"), ("sbm_cluster", "eigen")])
def test_c_abi_result_does_not_depend_on_the_outputs_contents(name, level, tmp_path, gpu, egt_lib):
    from egt_amd import _lib as L
    from egt_amd.device_data import batch_desc
    _, dev = _pair(DC.edge_case_store(tmp_path, name), name, level, gpu)
    sp = dev._splits["training"]
    ids = [4, 0, 12, 3, 5, 4]                                             # a record twice, the graphs without edges
    ref = dev.assemble("training", ids)
    N = ref["graph_matrix"].shape[1]
    assert N == 33
    desc = batch_desc(sp.kinds, len(ids), N, sp.records)
    idx = torch.tensor(ids, dtype=torch.int32, device=gpu)
    keys = dev._keys(sp)
    out = {f: torch.empty_like(ref[k]).view(torch.uint8).fill_(0xFF).view(ref[k].dtype).view(ref[k].shape) for k, f in keys}
    st = L.params_struct(L.BatchStore, L.BATCH_STORE_FIELDS, [sp.store.get(f) for f in L.BATCH_STORE_FIELDS])
    ot = L.params_struct(L.BatchOut, L.BATCH_OUT_FIELDS, [out.get(f) for f in L.BATCH_OUT_FIELDS])
    L.check(egt_lib.egt_batch_assemble(C.byref(desc), C.byref(st), L.ptr(idx), C.byref(ot), L.current_stream()))
    torch.cuda.synchronize()
    for k, f in keys:
        assert torch.equal(out[f].view(torch.int32), ref[k].view(torch.int32)), k
    # an index outside the split is an empty graph, not a read outside the store
    idx = torch.tensor([1, sp.records, -1, 2, 0, 6], dtype=torch.int32, device=gpu)
    L.check(egt_lib.egt_batch_assemble(C.byref(desc), C.byref(st), L.ptr(idx), C.byref(ot), L.current_stream()))
    torch.cuda.synchronize()
    assert out["num_nodes"].tolist() == [1, 0, 0, 16, 7, 7]
    assert torch.all(out["graph_matrix"][1:3] == 0) and torch.equal(out["node_features"][1], out["node_features"][2])


# ------------------------------------------------------------------------------------------------ training -----
def _train(cls, cfg, gpu, tmp_path, tag, on, graph=False, steps=3):
    torch.manual_seed(0)
    s = cls(dict(cfg, model_name=tag, save_path=str(tmp_path / tag), device_dataset=on, use_hipgraph=graph), device=gpu,
            print_fn=lambda *a: None)
    s.load_data()
    s.dataset._rng = np.random.default_rng(7)              # the epoch order: the host dataset's generator, on both paths
    s.dataset.prefetch_batch = False                       # the host batches are built on this thread, between the steps
    s.load_model()
    batches = []
    losses = []
    for b in itertools.islice(s.trainset, steps):
        batches.append({k: (v.detach().clone().to(gpu) if torch.is_tensor(v) else v) for k, v in b.items()})
        losses.append(s.train_step(b))
    assert (getattr(s, "device_dataset", None) is not None) == on
    return losses, [p.detach().clone() for p in s.params], batches


def _training_check(cls, scheme, name, gpu, tmp_path, graph=False, **extra):
    store = DC.write_store(tmp_path, name, DC.clean_records(name, 0), DC.clean_records(name, 1)[:5])
    cfg = dict(scheme=scheme, num_epochs=1, initial_lr=2e-3, batch_size=4, model_width=16, edge_width=16, model_height=1, upto_hop=4,
               random_mask_prob=0.0, dataset_path=store, **extra)
    off1, off2 = _train(cls, cfg, gpu, tmp_path, "off1", False, graph), _train(cls, cfg, gpu, tmp_path, "off2", False, graph)
    on = _train(cls, cfg, gpu, tmp_path, "on", True, graph)
    for hb, db in zip(off1[2], on[2]):                     # the batches, whatever the step does with them
        _same(hb, db, gpu, "training batch")
    repeatable = off1[0] == off2[0] and all(torch.equal(a, b) for a, b in zip(off1[1], off2[1]))
    assert repeatable, "the host-fed run is not bitwise repeatable: only the batches were compared"
    assert on[0] == off1[0]
    for a, b in zip(off1[1], on[1]):
        assert torch.equal(a, b)


def test_zinc_training_is_identical_with_the_device_dataset(tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    _training_check(T.ZincSVDScheme, "zinc.svd", "zinc", gpu, tmp_path, use_svd=False)


def test_pattern_training_is_identical_with_the_device_dataset(tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    _training_check(T.PatternSVDScheme, "pattern.svd", "sbm_pattern", gpu, tmp_path, num_svd_features=8, sel_svd_features=4)


def test_zinc_hipgraph_training_is_identical_with_the_device_dataset(tmp_path, gpu, egt_lib):
    from egt_amd import training as T
    _training_check(T.ZincSVDScheme, "zinc.svd", "zinc", gpu, tmp_path, graph=True, use_svd=False)
