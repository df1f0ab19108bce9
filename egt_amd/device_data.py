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

For the resident step (``config.resident_step``, egt_amd.graph.ResidentStep) a whole epoch goes to the device at once:
``epoch_plan`` draws the epoch from the same generator, copies its record indices to the split's device table and returns the
per-batch ``(B, N)``; ``assemble_at`` (egt_batch_assemble_at) then writes the batch at the table's device cursor into tensors
the caller owns (``static_batch``), from inside a captured graph.
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


def batch_shapes(desc: L.BatchDesc) -> Dict[str, tuple]:
    """egt_batch_out's fields -> (shape, torch dtype) for the descriptor, in the shapes of the header"""
    import torch
    B, N = desc.B, desc.N
    f32, i32 = torch.float32, torch.int32
    pe_tail = (desc.pe_features, 2) if desc.pe_kind == L.BATCH_PE_SVD else (desc.pe_features,)
    return dict(graph_matrix=((B, N, N), f32),
                feature_matrix=((B, N, N, 1), f32) if desc.edge_kind == L.BATCH_F32 else ((B, N, N), i32),
                node_features=((B, N, desc.node_width), f32) if desc.node_kind == L.BATCH_F32 else ((B, N), i32),
                pe=((B, N) + pe_tail, f32),
                target={L.BATCH_TGT_GRAPH_F32: ((B, 1), f32), L.BATCH_TGT_GRAPH_I32: ((B,), i32),
                        L.BATCH_TGT_NODE_I32: ((B, N), i32)}[desc.target_kind],
                num_nodes=((B,), i32))


def assemble_batch(desc: L.BatchDesc, store: Dict[str, "torch.Tensor"], idx, want: Sequence[str],
                   out: Optional[Dict[str, "torch.Tensor"]] = None, cursor=None) -> Dict[str, "torch.Tensor"]:
    """egt_batch_assemble on the current stream: ``store`` maps the fields of egt_batch_store to device tensors (absent =
    NULL), ``idx`` is the int32 device tensor of record indices, ``want`` names the outputs (egt_batch_out's fields).  The
    outputs are fresh tensors in the shapes of the header, or -- with ``out`` -- the caller's own tensors of those shapes
    (a captured step's static batch).  With ``cursor`` (a device int64 word) the call is egt_batch_assemble_at: ``idx`` is
    the index table and the batch is its B entries from ``*cursor`` on, read when the kernel runs."""
    import torch
    lib = L.load()
    if lib.egt_batch_supported(C.byref(desc)) != 1:
        lib.egt_batch_assemble(C.byref(desc), None, None, None, None)       # (leaves the reason)
        raise ValueError("egt_batch_assemble does not cover this batch: " + lib.egt_last_error_string().decode(errors="replace"))
    dev = idx.device
    shapes = batch_shapes(desc)
    if out is None:
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
    else:
        for k in want:
            t = out.get(k)
            if t is None or tuple(t.shape) != shapes[k][0] or t.dtype != shapes[k][1] or t.device != dev or not t.is_contiguous():
                raise ValueError(f"assemble_batch: out[{k!r}] must be a contiguous {shapes[k][1]} tensor of shape {shapes[k][0]} on {dev}")
        out = {k: out[k] for k in want}
    st = L.params_struct(L.BatchStore, L.BATCH_STORE_FIELDS, [store.get(f) for f in L.BATCH_STORE_FIELDS])
    ot = L.params_struct(L.BatchOut, L.BATCH_OUT_FIELDS, [out.get(f) for f in L.BATCH_OUT_FIELDS])
    if cursor is None:
        L.check(lib.egt_batch_assemble(C.byref(desc), C.byref(st), L.ptr(idx), C.byref(ot), L.current_stream()))
    else:
        if cursor.dtype != torch.int64 or cursor.numel() != 1 or cursor.device != dev:
            raise ValueError(f"assemble_batch: the cursor is one int64 word on {dev}")
        if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() < desc.B:
            raise ValueError(f"assemble_batch: the index table is a contiguous int32 tensor; one of {idx.numel()} entries cannot hold a batch of {desc.B}")
        L.check(lib.egt_batch_assemble_at(C.byref(desc), C.byref(st), L.ptr(idx), L.ptr(cursor), C.byref(ot), L.current_stream()))
    return out


class EpochPlan:
    """One epoch of a split for the resident step: ``ids`` (record indices in the epoch's order, int32), ``batches``
    [(B_i, N_i)] and ``offsets`` (where batch i starts in ``ids``); ``table`` is the device table the indices were copied
    to (``ids`` occupies its first len(ids) entries) and ``cursor`` the device word the captured steps read."""

    def __init__(self, split, ids, batches, table=None, cursor=None):
        self.split, self.ids, self.batches = split, ids, batches
        self.offsets = np.concatenate([[0], np.cumsum([b for b, _ in batches], dtype=np.int64)])[:-1].astype(np.int64) if batches \
            else np.zeros(0, np.int64)
        self.table, self.cursor = table, cursor

    def __len__(self):
        return len(self.batches)


def plan_epoch(host: GraphDataset, split: str, index: Dict[str, int], num_nodes: np.ndarray, batch_size: int,
               drop_remainder=False) -> EpochPlan:
    """One epoch of ``host.iter_tokens(split)`` -- the draws ``batches`` would make from the dataset's generator, in its order
    -- cut into batches of ``batch_size`` (a short last one unless ``drop_remainder``).  ``index`` maps a token to its record
    in the packed split, ``num_nodes`` is the host copy of the split's node counts: N_i is the batch's longest graph, or the
    dataset's fixed ``max_length``.  Host only."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    ids = np.fromiter((index[t] for t in host.iter_tokens(split)), np.int32)
    full = len(ids) // batch_size
    sizes = [batch_size] * full + ([len(ids) - full * batch_size] if len(ids) % batch_size and not drop_remainder else [])
    ids = ids[:sum(sizes)]
    fixed = None if host.max_length is None else int(host.max_length)
    batches, o = [], 0
    for b in sizes:
        longest = int(num_nodes[ids[o:o + b]].max())
        if fixed is not None and longest > fixed:
            raise ValueError(f"a record with {longest} nodes exceeds the padded shape ({fixed},)")
        batches.append((b, longest if fixed is None else fixed))
        o += b
    return EpochPlan(split, ids, batches)


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
        self.table = self.cursor = None              # epoch_plan: the split's index table and its cursor, made on first use
        self.staging = []                            # [pinned int32 buffer, event of its last copy] x 2
        self.plans = 0


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

    def assemble(self, split: str, ids: Sequence[int], out: Optional[dict] = None) -> dict:
        """the padded batch of the records ``ids`` (indices into the split, store order) as device tensors: fresh ones, or
        ``out`` (a ``static_batch`` of the batch's shape)"""
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
        out = assemble_batch(batch_desc(sp.kinds, len(ids), N, sp.records), sp.store, idx, [f for _, f in keys],
                             out=None if out is None else {f: out[k] for k, f in keys})
        return {k: out[f] for k, f in keys}

    # ---- the resident step: a whole epoch's indices on the device, batches written into the caller's tensors ----
    def plan_tokens(self, split: str, batch_size: int, drop_remainder=False) -> EpochPlan:
        """``plan_epoch`` over this dataset's split: host only, nothing is copied"""
        sp = self._splits[split]
        return plan_epoch(self.host, split, sp.index, sp.num_nodes_host, batch_size, drop_remainder)

    def epoch_plan(self, split: str, batch_size: int, drop_remainder=False) -> EpochPlan:
        """``plan_tokens`` with the indices in the split's persistent device table (one asynchronous copy from pinned memory on
        the current stream) and the split's cursor set to 0.  Two pinned buffers take turns and each waits for the event of
        its last copy, so a buffer is never rewritten before that copy has run; the host never waits for the GPU unless two
        plans are still in flight."""
        import torch
        plan = self.plan_tokens(split, batch_size, drop_remainder)
        sp = self._splits[split]
        if sp.table is None:
            sp.table = torch.zeros(max(sp.records, 1), dtype=torch.int32, device=self.device)
            sp.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
            sp.staging = [[torch.empty(max(sp.records, 1), dtype=torch.int32).pin_memory(), None] for _ in range(2)]
        slot = sp.staging[sp.plans % 2]
        sp.plans += 1
        if slot[1] is not None and not slot[1].query():
            slot[1].synchronize()                    # (the copy of two plans ago: long done unless epochs are a few steps long)
        n = len(plan.ids)
        slot[0].numpy()[:n] = plan.ids
        sp.table[:n].copy_(slot[0][:n], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        sp.cursor.zero_()
        plan.table, plan.cursor = sp.table, sp.cursor
        return plan

    def batch_keys(self, split: str) -> List[Tuple[str, str]]:
        return self._keys(self._splits[split])

    def static_batch(self, split: str, B: int, N: int) -> dict:
        """uninitialised tensors of one (B, N) batch, keyed as the batches are: what ``assemble_at`` writes into"""
        import torch
        sp = self._splits[split]
        shapes = batch_shapes(batch_desc(sp.kinds, B, N, sp.records))
        return {k: torch.empty(shapes[f][0], dtype=shapes[f][1], device=self.device) for k, f in self._keys(sp)}

    def assemble_at(self, plan: EpochPlan, B: int, N: int, out: dict) -> dict:
        """the batch of the B records at the plan's cursor, written into ``out`` (a ``static_batch``): one launch of
        egt_batch_assemble_at on the current stream, capturable; the cursor is not moved"""
        sp = self._splits[plan.split]
        keys = self._keys(sp)
        assemble_batch(batch_desc(sp.kinds, B, N, sp.records), sp.store, plan.table, [f for _, f in keys],
                       out={f: out[k] for k, f in keys}, cursor=plan.cursor)
        return out

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
