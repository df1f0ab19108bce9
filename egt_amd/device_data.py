"""Device-resident datasets: a split's PACKED records live in HBM and one HIP launch (egt_batch_assemble,
csrc/egt_batch.hip) writes the padded tensors of a batch from the B record indices.

``pack_split`` (host only) turns one pass over a split into flat arrays: per record the node count, the edges stably sorted
by source row with a per-node row offset, the node rows, the edge features in the sorted order, the positional-encoding rows
(the same ``svd_features`` / ``eigen_features`` calls the host path makes) and the target.  ``DeviceGraphDataset`` -- what
``GraphDataset.to_device(device)`` returns -- uploads every split once and offers ``get_batched_data`` / ``batches`` with the
host's signature: the epoch order is the host dataset's own token generator (same draws from the same generator), and the
batches equal the host's bit for bit, with the same keys, dtypes and shapes.  Per batch the host does index arithmetic on B
integers, takes N from a host copy of the node counts, copies the indices from a pinned buffer and launches; it never
synchronises.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .data import GraphDataset, _Epochs, get_adjacency
from .dp import shard_batch

MAX_NODES = 512                    # egt_batch_supported: 1 <= N <= 512
STORE_FIELDS = L.BATCH_STORE_FIELDS


def _kinds(ds: GraphDataset) -> dict:
    """the descriptor fields that follow from the dataset's spec and level"""
    fields = {f.name: f for f in ds.spec.fields}
    nf, tg = fields["node_features"], fields["target"]
    node_kind = L.BATCH_F32 if np.dtype(nf.dtype).kind == "f" else L.BATCH_I32
    node_width = int(np.prod(nf.shape[1:], dtype=np.int64)) if len(nf.shape) > 1 else 1
    edge_kind = L.BATCH_NONE
    if ds.spec.fm_tail is not None:
        edge_kind = L.BATCH_F32 if np.dtype(fields["edge_features"].dtype).kind == "f" else L.BATCH_I32
    if tg.shape == (None,):
        target_kind = L.BATCH_TGT_NODE_I32
    else:
        target_kind = L.BATCH_TGT_GRAPH_F32 if np.dtype(tg.dtype).kind == "f" else L.BATCH_TGT_GRAPH_I32
    pe_kind = {"svd": L.BATCH_PE_SVD, "eigen": L.BATCH_PE_EIGEN}.get(ds.level, L.BATCH_PE_NONE)
    return dict(node_kind=node_kind, node_width=node_width, edge_kind=edge_kind, edge_width=0 if edge_kind == L.BATCH_NONE else 1,
                pe_kind=pe_kind, pe_features=0 if pe_kind == L.BATCH_PE_NONE else int(ds.num_features), target_kind=target_kind,
                flags=L.BATCH_MARK_INVALID if ds.mark_invalid_features else 0,
                matrix_pad=float(np.float32(ds.matrix_pad_value)), mask_f=float(np.float32(ds.mask_value)),
                mask_i=int(np.asarray(ds.mask_value).astype(np.int32)))


def _pe_name(ds: GraphDataset) -> Optional[str]:
    return {"svd": "singular_vectors", "eigen": "eigen_vectors"}.get(ds.level)


def pack_split(ds: GraphDataset, split: str, with_pe: bool = True) -> Dict[str, np.ndarray]:
    """One pass over the records of ``split`` -> the arrays of egt_batch_store (include/egt_amd.h), as numpy arrays, plus
    ``tokens`` (the split's record tokens in store order: record r of the arrays is tokens[r]).  Host only."""
    ds.load_data()
    k = _kinds(ds)
    if not with_pe:
        k.update(pe_kind=L.BATCH_PE_NONE, pe_features=0)
    tokens = list(ds.record_tokens[split])
    num_nodes, row_off, edge_dst, edge_feat, node_rows, pe_rows, targets = [], [], [], [], [], [], []
    n_edges = []
    for tok in tokens:
        rec = ds._raw_record(tok)
        n = int(rec["num_nodes"])
        edges = np.asarray(rec["edges"]).reshape(-1, 2)
        if len(edges) and (edges.min() < 0 or edges.max() >= n):
            raise ValueError(f"{tok}: an edge names a node outside 0..{n - 1}")
        nf = np.asarray(rec["node_features"])
        if nf.shape[0] != n:
            raise ValueError(f"{tok}: {nf.shape[0]} node rows for num_nodes = {n}")
        order = np.argsort(edges[:, 0], kind="stable")           # duplicates of one (i,j) keep the edge list's order
        counts = np.bincount(edges[:, 0], minlength=n)
        num_nodes.append(n)
        n_edges.append(len(edges))
        row_off.append(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
        edge_dst.append(edges[order, 1].astype(np.int32))
        node_rows.append(nf.reshape(n, k["node_width"]))
        if k["edge_kind"] != L.BATCH_NONE:
            ef = np.asarray(rec["edge_features"])
            if ef.size != len(edges):
                raise ValueError(f"{tok}: {ef.size} edge-feature values for {len(edges)} edges (one value per edge is covered)")
            edge_feat.append(ef.reshape(-1)[order])
        if k["pe_kind"] != L.BATCH_PE_NONE:
            width = k["pe_features"] * (2 if k["pe_kind"] == L.BATCH_PE_SVD else 1)
            rows = np.zeros((n, width), np.float32)
            if n:
                adj = get_adjacency(edges, n, ds.normalize, ds.symmetric, True) if ds.level == "svd" else None
                v = np.asarray(ds._pe_features(rec, n, adj)[_pe_name(ds)], np.float32)
                if ds.level == "eigen":                         # a graph with fewer than F + 1 nodes has fewer columns: collate pads them
                    rows[:, :v.shape[1]] = v
                else:
                    rows[:] = v.reshape(n, width)
            pe_rows.append(rows)
        tg = np.asarray(rec["target"])
        if k["target_kind"] == L.BATCH_TGT_NODE_I32 and tg.shape[0] != n:
            raise ValueError(f"{tok}: {tg.shape[0]} node targets for num_nodes = {n}")
        targets.append(tg.reshape(-1))
    cat = lambda xs, dt, tail=(): (np.concatenate(xs).astype(dt, copy=False) if xs else np.zeros((0,) + tail, dt))
    off = lambda xs: np.concatenate([[0], np.cumsum(xs, dtype=np.int64)]).astype(np.int64)
    ndt = np.float32 if k["node_kind"] == L.BATCH_F32 else np.int32
    out = dict(tokens=tokens, desc=k,
               num_nodes=np.asarray(num_nodes, np.int32), node_off=off(num_nodes), edge_off=off(n_edges),
               row_off=cat(row_off, np.int32), edge_dst=cat(edge_dst, np.int32),
               node_rows=cat(node_rows, ndt, (k["node_width"],)),
               targets=cat(targets, np.float32 if k["target_kind"] == L.BATCH_TGT_GRAPH_F32 else np.int32))
    if k["edge_kind"] != L.BATCH_NONE:
        out["edge_feat"] = cat(edge_feat, np.float32 if k["edge_kind"] == L.BATCH_F32 else np.int32)
    if k["pe_kind"] != L.BATCH_PE_NONE:
        out["pe_rows"] = cat(pe_rows, np.float32)
    return out


def batch_desc(kinds: dict, B: int, N: int, records: int) -> L.BatchDesc:
    return L.BatchDesc(B=B, N=N, records=records, **kinds)


def assemble_batch(desc: L.BatchDesc, store: Dict[str, "torch.Tensor"], idx, want: Sequence[str]) -> Dict[str, "torch.Tensor"]:
    """egt_batch_assemble on the current stream: ``store`` maps the fields of egt_batch_store to device tensors (absent =
    NULL), ``idx`` is the int32 device tensor of record indices, ``want`` names the outputs (egt_batch_out's fields).  The
    outputs are fresh tensors in the shapes of the header."""
    import torch
    lib = L.load()
    if lib.egt_batch_supported(C.byref(desc)) != 1:
        lib.egt_batch_assemble(C.byref(desc), None, None, None, None)       # (leaves the reason)
        raise ValueError("egt_batch_assemble does not cover this batch: " + lib.egt_last_error_string().decode(errors="replace"))
    B, N, dev = desc.B, desc.N, idx.device
    f32, i32 = torch.float32, torch.int32
    pe_tail = (desc.pe_features, 2) if desc.pe_kind == L.BATCH_PE_SVD else (desc.pe_features,)
    shapes = dict(graph_matrix=((B, N, N), f32),
                  feature_matrix=((B, N, N, 1), f32) if desc.edge_kind == L.BATCH_F32 else ((B, N, N), i32),
                  node_features=((B, N, desc.node_width), f32) if desc.node_kind == L.BATCH_F32 else ((B, N), i32),
                  pe=((B, N) + pe_tail, f32),
                  target={L.BATCH_TGT_GRAPH_F32: ((B, 1), f32), L.BATCH_TGT_GRAPH_I32: ((B,), i32),
                          L.BATCH_TGT_NODE_I32: ((B, N), i32)}[desc.target_kind],
                  num_nodes=((B,), i32))
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
    st = L.params_struct(L.BatchStore, L.BATCH_STORE_FIELDS, [store.get(f) for f in L.BATCH_STORE_FIELDS])
    ot = L.params_struct(L.BatchOut, L.BATCH_OUT_FIELDS, [out.get(f) for f in L.BATCH_OUT_FIELDS])
    L.check(lib.egt_batch_assemble(C.byref(desc), C.byref(st), L.ptr(idx), C.byref(ot), L.current_stream()))
    return out


class _Split:
    """one split on the device: the store's tensors, a host copy of the node counts, token -> record index"""

    def __init__(self, packed: dict, device):
        import torch
        self.kinds = packed["desc"]
        self.records = len(packed["tokens"])
        self.index = {t: i for i, t in enumerate(packed["tokens"])}
        self.num_nodes_host = packed["num_nodes"]
        self.store = {f: torch.from_numpy(np.ascontiguousarray(packed[f])).to(device) for f in STORE_FIELDS if f in packed}
        self.nbytes = sum(t.numel() * t.element_size() for t in self.store.values())


class DeviceGraphDataset:
    """``GraphDataset.to_device(device)``: the host dataset's batches, assembled on the device."""

    def __init__(self, host: GraphDataset, device):
        import torch
        self.host, self.device = host, torch.device(device)
        if host.level == "records":
            raise ValueError('level "records" has no padded matrices: it stays on the host')
        for name in ("normalize", "symmetric", "laplacian"):
            if getattr(host, name):
                raise ValueError(f"{name}=True is not covered by the device-resident dataset (no scheme sets it)")
        for flag, name, applies in (("return_edges", "edges", True), ("return_edge_features", "edge_features", host.spec.fm_tail is not None),
                                    ("return_sing_vals", "singular_values", host.level == "svd")):
            if applies and name not in host._dropped:
                raise ValueError(f"{flag}=True is not covered by the device-resident dataset")
        if self.device.type != "cuda":
            raise ValueError(f"a device-resident dataset needs a GPU (got device {device!r})")
        host.load_data()
        with_pe = _pe_name(host) is not None and _pe_name(host) not in host._excluded     # (an excluded encoding is never computed)
        self._splits = {s: _Split(pack_split(host, s, with_pe), self.device) for s in host.splits}

    # ---- the host dataset's surface ----
    @property
    def splits(self):
        return self.host.splits

    @property
    def record_tokens(self):
        return self.host.record_tokens

    @property
    def nbytes(self) -> int:
        """bytes of device memory the packed splits occupy"""
        return sum(s.nbytes for s in self._splits.values())

    def load_data(self):
        self.host.load_data()
        return self

    def exclude(self, names):
        self.host.exclude(names)

    # ---- batches ----
    def _keys(self, sp: _Split) -> List[Tuple[str, str]]:
        """(batch key, egt_batch_out field) in the order of the host's batch dictionary"""
        h = self.host
        keys = [("num_nodes", "num_nodes"), ("node_features", "node_features"), ("target", "target"), ("graph_matrix", "graph_matrix")]
        if h.spec.fm_tail is not None:
            keys.append(("feature_matrix", "feature_matrix"))
        if _pe_name(h) is not None:
            keys.append((_pe_name(h), "pe"))
        gone = h._dropped | h._excluded
        keys = [kf for kf in keys if kf[0] not in gone]
        if any(f == "pe" for _, f in keys) and sp.kinds["pe_kind"] == L.BATCH_PE_NONE:
            raise ValueError(f"{_pe_name(h)} was excluded when the dataset went to the device: its rows were never computed")
        return keys

    def assemble(self, split: str, ids: Sequence[int]) -> dict:
        """the padded batch of the records ``ids`` (indices into the split, store order) as device tensors"""
        import torch
        sp = self._splits[split]
        ids = np.asarray(ids, np.int32)
        longest = int(sp.num_nodes_host[ids].max())
        N = longest if self.host.max_length is None else int(self.host.max_length)
        if longest > N:
            raise ValueError(f"a record with {longest} nodes exceeds the padded shape ({N},)")
        staged = torch.empty(len(ids), dtype=torch.int32, pin_memory=True)    # (the pinned-memory cache holds it until the copy ran)
        staged.numpy()[:] = ids
        idx = staged.to(self.device, non_blocking=True)
        keys = self._keys(sp)
        out = assemble_batch(batch_desc(sp.kinds, len(ids), N, sp.records), sp.store, idx, [f for _, f in keys])
        return {k: out[f] for k, f in keys}

    def _finish(self, split, ids, map_fn, shard, train):
        counts = None
        if shard is not None:           # GraphDataset._finish's rules for a short last batch
            n_global = len(ids)
            if n_global < shard[1] and train:
                return None
            lo, hi = shard_batch(n_global, shard[1], shard[0])
            if hi == lo:
                return None
            ids = ids[lo:hi]
            counts = (hi - lo, n_global)
        b = self.assemble(split, ids)
        if counts is not None:
            b["_local_count"], b["_global_count"] = counts
        return map_fn(b) if map_fn is not None else b

    def batches(self, split: str, batch_size: int, drop_remainder=False, map_fn: Optional[Callable] = None,
                shard: Optional[Tuple[int, int]] = None, as_torch=True, device=None, collective: Optional[bool] = None) -> Iterator:
        """GraphDataset.batches on the device: the same batches in the same order for the same seed"""
        import torch
        if not as_torch:
            raise ValueError("a device-resident dataset yields torch tensors (as_torch=False is the host dataset's)")
        if device is not None and torch.device(device).type != self.device.type:
            raise ValueError(f"the dataset is resident on {self.device}, not on {device!r}")
        train = (split == "training") if collective is None else bool(collective)
        index = self._splits[split].index

        def gen():
            cur: List[int] = []
            for t in self.host.iter_tokens(split):
                cur.append(index[t])
                if len(cur) == batch_size:
                    b = self._finish(split, cur, map_fn, shard, train)
                    if b is not None:
                        yield b
                    cur = []
            if cur and not drop_remainder:
                b = self._finish(split, cur, map_fn, shard, train)
                if b is not None:
                    yield b
        return gen()

    def get_batched_data(self, batch_size, drop_remainder=False, map_fns=None, **kw):
        """per split an object whose iteration is one (reshuffled) epoch, as GraphDataset.get_batched_data"""
        def per_split(v):
            return v if isinstance(v, dict) else {s: v for s in self.splits}
        bs, dr, mf = per_split(batch_size), per_split(drop_remainder), per_split(map_fns)
        self.load_data()
        out = tuple(_Epochs(self, s, bs[s], dr[s], mf[s], kw) for s in self.splits)
        return out if len(out) > 1 else out[0]
