"""Device-resident datasets, the host side (egt_amd/device_data.py, include/egt_amd.h: egt_batch_*): struct layouts, the packed
store's invariants, the shared epoch order, the config key and the refusals -- all without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import device_data_cases as DC
from egt_amd import data as D
from egt_amd import training as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_the_ctypes_mirrors_and_the_symbols_exist(tmp_path, egt_lib):
    from egt_amd import _lib as L
    pairs = [("egt_batch_desc", L.BatchDesc), ("egt_batch_store", L.BatchStore), ("egt_batch_out", L.BatchOut)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("abi %d\\n", EGT_ABI_VERSION);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert int(got["abi"]) == 4 == L.ABI_VERSION
    header = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    for name in ("egt_batch_supported", "egt_batch_assemble"):
        assert name in L._PROTOS and getattr(egt_lib, name) is not None and f"int {name}(" in header
    assert L.BatchStore._fields_ == [(f, C.c_void_p) for f in L.BATCH_STORE_FIELDS]
    assert L.BatchOut._fields_ == [(f, C.c_void_p) for f in L.BATCH_OUT_FIELDS]


def test_supported_and_argument_validation_without_gpu(egt_lib):
    from egt_amd import _lib as L
    from egt_amd.device_data import MAX_NODES
    ok = dict(B=4, N=37, records=13, node_kind=L.BATCH_I32, node_width=1, edge_kind=L.BATCH_I32, edge_width=1, pe_kind=L.BATCH_PE_SVD,
              pe_features=8, target_kind=L.BATCH_TGT_GRAPH_F32, flags=L.BATCH_MARK_INVALID, matrix_pad=0.0, mask_f=-1.0, mask_i=-1)
    sup = lambda **kw: egt_lib.egt_batch_supported(C.byref(L.BatchDesc(**dict(ok, **kw))))
    assert sup() == 1 and sup(N=MAX_NODES) == 1 and sup(N=1) == 1
    assert sup(N=MAX_NODES + 1) == 0 and sup(N=0) == 0 and sup(B=0) == 0 and sup(records=0) == 0
    assert sup(node_kind=L.BATCH_F32, node_width=5) == 1 and sup(node_width=5) == 0          # int32 node rows have one word
    assert sup(edge_kind=L.BATCH_NONE, edge_width=0) == 1 and sup(edge_kind=L.BATCH_F32, edge_width=2) == 0
    assert sup(pe_kind=L.BATCH_PE_NONE, pe_features=0) == 1 and sup(pe_features=33) == 0 and sup(pe_kind=L.BATCH_PE_EIGEN, pe_features=33) == 1
    assert sup(target_kind=3) == 0 and sup(flags=2) == 0
    d = L.BatchDesc(**ok)
    assert egt_lib.egt_batch_assemble(C.byref(d), None, None, None, None) == L.EGT_E_NULL
    st, out = L.BatchStore(), L.BatchOut()
    assert egt_lib.egt_batch_assemble(C.byref(d), C.byref(st), C.c_void_p(256), C.byref(out), None) == L.EGT_E_NULL   # store.num_nodes
    d.N = 600
    assert egt_lib.egt_batch_assemble(C.byref(d), C.byref(st), C.c_void_p(256), C.byref(out), None) == L.EGT_E_SHAPE
    assert b"outside 1..512" in egt_lib.egt_last_error_string()


@pytest.mark.parametrize("name", ["zinc", "cifar10", "sbm_pattern"])
def test_pack_split_invariants(name, tmp_path):
    from egt_amd import _lib as L
    from egt_amd.device_data import pack_split
    recs = DC.edge_case_records(name, 0)
    ds = D.GraphDataset(name, DC.edge_case_store(tmp_path, name), level="svd", return_mat=True, num_features=4)
    p = pack_split(ds, "training")
    R = len(recs)
    assert len(p["tokens"]) == R == 13 and p["tokens"] == ds.record_tokens["training"]
    assert np.array_equal(p["num_nodes"], [r["num_nodes"] for r in recs]) and p["num_nodes"].dtype == np.int32
    for off, counts in ((p["node_off"], p["num_nodes"]), (p["edge_off"], [len(r["edges"]) for r in recs])):
        assert off.dtype == np.int64 and off.shape == (R + 1,) and off[0] == 0
        assert np.all(np.diff(off) >= 0) and np.array_equal(np.diff(off), counts)               # monotone, one span per record
    assert p["row_off"].shape == (p["node_off"][-1] + R,) and p["edge_dst"].shape == (p["edge_off"][-1],)
    assert p["pe_rows"].shape == (p["node_off"][-1], 8) and p["pe_rows"].dtype == np.float32
    for r, rec in enumerate(recs):
        n, e = int(rec["num_nodes"]), rec["edges"]
        ro = p["row_off"][p["node_off"][r] + r: p["node_off"][r] + r + n + 1]
        assert ro[0] == 0 and ro[-1] == len(e) and np.all(np.diff(ro) >= 0)                      # row offsets cover the record's edges
        dst = p["edge_dst"][p["edge_off"][r]: p["edge_off"][r + 1]]
        feat = p["edge_feat"][p["edge_off"][r]: p["edge_off"][r + 1]] if "edge_feat" in p else None
        for i in range(n):
            mine = np.flatnonzero(e[:, 0] == i)                                                    # row i's edges IN LIST ORDER: the sort is stable
            assert np.array_equal(dst[ro[i]:ro[i + 1]], e[mine, 1])
            if feat is not None:
                assert np.array_equal(feat[ro[i]:ro[i + 1]], rec["edge_features"].reshape(-1)[mine])
        host = ds.record("training", p["tokens"][r])
        assert np.array_equal(p["pe_rows"][p["node_off"][r]: p["node_off"][r + 1]].reshape(n, 4, 2), host["singular_vectors"])
        assert np.array_equal(p["node_rows"][p["node_off"][r]: p["node_off"][r + 1]].reshape(rec["node_features"].shape), rec["node_features"])
    # the record with duplicated edges: (4,1) three times, (2,5) twice, in the order of the list
    e0 = recs[0]["edges"]
    assert (e0 == [4, 1]).all(1).sum() >= 3 and (e0 == [2, 5]).all(1).sum() >= 2 and (e0 == [3, 3]).all(1).sum() >= 1
    if name == "cifar10":       # ... and the host's sum over the (4,1) duplicates depends on that order (the data can tell a reordering)
        f = recs[0]["edge_features"][(e0 == [4, 1]).all(1), 0]
        fwd = rev = np.float32(0)
        for a, b in zip(f, f[::-1]):
            fwd, rev = fwd + (a + np.float32(1)), rev + (b + np.float32(1))
        assert fwd != rev and ds.record("training", p["tokens"][0])["feature_matrix"][4, 1, 0] == fwd - np.float32(1)
    k = p["desc"]
    assert k["target_kind"] == {"zinc": L.BATCH_TGT_GRAPH_F32, "cifar10": L.BATCH_TGT_GRAPH_I32, "sbm_pattern": L.BATCH_TGT_NODE_I32}[name]
    assert p["targets"].shape == ((p["node_off"][-1],) if name == "sbm_pattern" else (R,))
    bad = [dict(r) for r in recs]
    bad[2]["edges"] = bad[2]["edges"].copy(); bad[2]["edges"][0, 1] = 16                          # a destination outside the graph
    bad_ds = D.GraphDataset(name, DC.write_store(tmp_path, name, bad, bad[:2], "_bad"), level="matrix")
    with pytest.raises(ValueError, match="outside"):
        pack_split(bad_ds, "training")


def test_token_order_is_shared_and_the_host_sequence_is_unchanged(tmp_path):
    path = DC.edge_case_store(tmp_path, "zinc")
    mk = lambda seed: D.GraphDataset("zinc", path, level="matrix", max_shuffle_len=5, seed=seed, prefetch_batch=False)
    a, b, c = mk(9), mk(9), mk(9)
    names = lambda ds: [r["record_name"].decode() for r in ds.iter_records("training")]
    for _ in range(2):                                     # two epochs: the generator's state carries over
        ra, tb = names(a), list(b.iter_tokens("training"))
        assert ra == tb and sorted(ra) == sorted(a.record_tokens["training"]) and ra != a.record_tokens["training"]
    # the draws are the ones iter_records always made: shuffle, then one integer per emitted record
    c.load_data()
    toks = list(c.record_tokens["training"])
    rng = np.random.default_rng(9)
    rng.shuffle(toks)
    buf, want = [], []
    for t in toks:
        if len(buf) < 5:
            buf.append(t)
            continue
        j = int(rng.integers(len(buf)))
        want.append(buf[j]); buf[j] = t
    while buf:
        j = int(rng.integers(len(buf)))
        buf[j], buf[-1] = buf[-1], buf[j]
        want.append(buf.pop())
    assert names(c) == want
    assert list(c.iter_tokens("validation")) == c.record_tokens["validation"]          # never shuffled


def test_config_key_and_refusals(tmp_path):
    assert T.default_config()["device_dataset"] is False
    c = T.make_config({"device_dataset": True})
    assert c.device_dataset is True and c.fused_optimizer is False and c.use_hipgraph is False
    for scheme in T.SCHEMES:
        assert T.make_config({"scheme": scheme}).device_dataset is False
    path = DC.edge_case_store(tmp_path, "zinc")
    cfg = dict(scheme="zinc.svd", model_width=16, edge_width=16, model_height=1, use_svd=False, device_dataset=True,
               dataset_path=path, save_path=str(tmp_path / "run"))
    from test_training import _Stub
    for device in (None, "cpu"):
        with pytest.raises(ValueError, match="device_dataset needs"):
            T.ZincSVDScheme(cfg, model_factory=_Stub, device=device).load_data()
        with pytest.raises(ValueError, match="device_dataset needs"):
            T.ZincSVDScheme(cfg, model_factory=_Stub, device=device).load_model()
    # to_device: what no scheme sets stays on the host
    for kw in (dict(normalize=True), dict(symmetric=True), dict(laplacian=True), dict(return_edges=True),
               dict(return_edge_features=True), dict(level="svd", return_sing_vals=True), dict(level="records")):
        ds = D.GraphDataset("zinc", path, **dict(dict(level="matrix"), **kw))
        with pytest.raises(ValueError, match="device-resident|stays on the host"):
            ds.to_device("cuda")
    with pytest.raises(ValueError, match="needs a GPU"):
        D.GraphDataset("zinc", path, level="matrix").to_device("cpu")
