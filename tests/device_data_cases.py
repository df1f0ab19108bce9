"""Synthetic packed stores for the device-resident dataset tests (tests/test_device_data_*.py).  No test functions here.

``edge_case_records``: thirteen graphs with n in {1, 2, 7, 16, 17, 33}; among them a graph without edges, edge lists in
scrambled order, an (i,j) that appears twice, an (i,j) that appears three times with distinct features (float features whose
sum depends on the order of the additions), and a self-loop edge in the list.  ``clean_records``: graphs a model can train
on (every pair at most once, feature values inside the embedding tables)."""
import numpy as np

from egt_amd import data as D

SIZES = (7, 1, 16, 2, 33, 17, 7, 16, 33, 2, 17, 7, 1)          # thirteen graphs
LEVELS = {"zinc": ("matrix", "svd", "eigen"), "zinc_full": ("matrix", "svd", "eigen"), "sbm_pattern": ("matrix", "svd", "eigen"),
          "sbm_cluster": ("matrix", "svd", "eigen"), "cifar10": ("matrix", "svd"), "mnist": ("matrix", "svd")}
# three features whose fp32 sum of (feature + 1) depends on the order of the additions: 2^24 absorbs the 0.5 that follows it
# (list order: ((2^24 + 0.5) - 16777215) - 1 = 0; reversed: ((-16777215 + 0.5) + 2^24) - 1 = 1)
ORDERED = (np.float32(16777216.0), np.float32(-0.5), np.float32(-16777216.0))


def _fields(name):
    return {f.name: f for f in D.SPECS[name].fields}


def _features(name, rng, n, n_edges):
    """node rows, edge features (None without), target of one record of dataset `name`"""
    f = _fields(name)
    nf_f, tg = f["node_features"], f["target"]
    if np.dtype(nf_f.dtype).kind == "f":
        nf = rng.standard_normal((n,) + tuple(nf_f.shape[1:])).astype(np.float32)
    else:
        nf = rng.integers(0, 3, size=n).astype(np.int32)
    ef = None
    if "edge_features" in f:
        e_f = f["edge_features"]
        if np.dtype(e_f.dtype).kind == "f":
            ef = rng.standard_normal((n_edges, 1)).astype(np.float32)
        else:
            ef = rng.integers(0, 3, size=n_edges).astype(np.int32)
    if tg.shape == (None,):
        target = rng.integers(0, 2, size=n).astype(np.int32)
    elif np.dtype(tg.dtype).kind == "f":
        target = np.asarray([rng.standard_normal()], np.float32)
    else:
        target = np.int32(rng.integers(0, 10))
    return nf, ef, target


def _record(name, rng, n, edges):
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    nf, ef, target = _features(name, rng, n, len(edges))
    rec = dict(num_nodes=np.int32(n), edges=edges, node_features=nf, target=target)
    if ef is not None:
        rec["edge_features"] = ef
    return rec


def _random_edges(rng, n, count):
    return rng.integers(0, n, size=(count, 2)).astype(np.int32)        # scrambled order, duplicates and self loops as they fall


def edge_case_records(name, seed=0, sizes=SIZES):
    rng = np.random.default_rng(seed)
    recs = []
    for g, n in enumerate(sizes):
        if g == 3 or n == 1 and g == 12:
            edges = np.zeros((0, 2), np.int32)                           # graphs without edges (n = 2 and the last n = 1)
        elif n == 1:
            edges = np.asarray([[0, 0], [0, 0]], np.int32)               # one node: a self loop, twice
        else:
            edges = _random_edges(rng, n, 3 * n)
        rec = _record(name, rng, n, edges)
        if g == 0:      # (2,5) twice, (4,1) three times -- apart from each other, between other edges -- and a self loop (3,3)
            e = np.concatenate([[[2, 5], [4, 1], [6, 0]], rec["edges"][:6], [[4, 1], [2, 5], [3, 3]], rec["edges"][6:12], [[4, 1]]]).astype(np.int32)
            rec = _record(name, rng, n, e)
            if "edge_features" in rec and rec["edge_features"].dtype == np.float32:
                for k, v in zip((1, 9, len(e) - 1), ORDERED):          # the three (4,1) edges
                    rec["edge_features"][k, 0] = v
        recs.append(rec)
    return recs


def clean_records(name, seed=0, sizes=(7, 9, 16, 12, 33, 17, 8, 16, 21, 5, 17, 7, 11)):
    """chains plus a few chords, both directions, every pair once, edge list scrambled"""
    rng = np.random.default_rng(seed)
    recs = []
    for n in sizes:
        pairs = {(i, i + 1) for i in range(n - 1)}
        for _ in range(n // 3):
            i, j = sorted(int(x) for x in rng.integers(0, n, size=2))
            if i != j:
                pairs.add((i, j))
        pairs = sorted(pairs)
        edges = np.asarray(pairs + [(j, i) for i, j in pairs], np.int32)
        half = len(pairs)
        nf, ef, target = _features(name, rng, n, half)
        rec = dict(num_nodes=np.int32(n), edges=edges, node_features=nf, target=target)
        if ef is not None:
            rec["edge_features"] = np.concatenate([ef, ef])
        perm = rng.permutation(len(edges))
        rec["edges"] = rec["edges"][perm]
        if ef is not None:
            rec["edge_features"] = rec["edge_features"][perm]
        recs.append(rec)
    return recs


def write_store(tmp_path, name, training, validation, tag=""):
    spec = D.SPECS[name]
    path = str(tmp_path / f"{name}{tag}.npz")
    D.write_packed_store(path, spec.db_name, dict(training=training, validation=validation),
                         {f.name: f.key for f in spec.fields}, meta=dict(num_graphs=len(training) + len(validation)))
    return path


def edge_case_store(tmp_path, name):
    return write_store(tmp_path, name, edge_case_records(name, 0), edge_case_records(name, 1, SIZES[:5]))


def big_records(name, sizes, seed=5):
    rng = np.random.default_rng(seed)
    return [_record(name, rng, n, _random_edges(rng, n, 4 * n)) for n in sizes]
