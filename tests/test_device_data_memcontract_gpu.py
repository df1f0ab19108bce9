"""The buffer contract of include/egt_amd.h for egt_batch_assemble, through the harness of tests/memcontract.py: the store's
arrays, the indices and every output in a guarded arena of exactly its byte count; outputs prefilled with 0x00 and with 0xFF;
NULL for the outputs that are not asked for.  Run Z is held to the Python wrapper's result bit for bit
(tests/test_device_data_gpu.py ties that result to the host pipeline)."""
import ctypes as C

import pytest
import torch

import device_data_cases as DC
import memcontract as M
from memcontract import Buf, Case, IN, OUT

pytestmark = pytest.mark.gpu
# (dataset, level, record indices, outputs left NULL)
CASES = {"zinc_svd": ("zinc", "svd", (4, 0, 12, 3, 5), ()),
         "zinc_matrix_only": ("zinc", "matrix", (8, 1, 2), ("node_features", "target", "num_nodes")),
         "cifar10_svd": ("cifar10", "svd", (0, 4, 3, 9, 10, 6, 2), ()),
         "cifar10_no_matrices": ("cifar10", "svd", (4, 7, 1), ("graph_matrix", "feature_matrix")),
         "pattern_eigen": ("sbm_pattern", "eigen", (5, 12, 8, 0), ()),
         "cluster_matrix_no_adjacency": ("sbm_cluster", "matrix", (2, 3, 4), ("graph_matrix",))}


def batch_case(lib, cid, tmp_path):
    from egt_amd import _lib as L
    from egt_amd import data as D
    from egt_amd.device_data import assemble_batch, batch_desc, pack_split
    name, level, ids, null = CASES[cid]
    kw = dict(return_mat=True) if level == "svd" else {}
    ds = D.GraphDataset(name, DC.edge_case_store(tmp_path, name), level=level, num_features=4, **kw)
    p = pack_split(ds, "training")
    kinds, B = p["desc"], len(ids)
    N = int(p["num_nodes"][list(ids)].max())
    desc = batch_desc(kinds, B, N, len(p["tokens"]))
    store = {f: torch.from_numpy(p[f]) for f in L.BATCH_STORE_FIELDS if f in p}
    f32, i32 = torch.float32, torch.int32
    pe_tail = {L.BATCH_PE_SVD: (4, 2), L.BATCH_PE_EIGEN: (4,)}.get(kinds["pe_kind"])
    outs = dict(graph_matrix=(f32, (B, N, N)), num_nodes=(i32, (B,)),
                node_features=(f32, (B, N, kinds["node_width"])) if kinds["node_kind"] == L.BATCH_F32 else (i32, (B, N)),
                target={L.BATCH_TGT_GRAPH_F32: (f32, (B, 1)), L.BATCH_TGT_GRAPH_I32: (i32, (B,)), L.BATCH_TGT_NODE_I32: (i32, (B, N))}[kinds["target_kind"]])
    if kinds["edge_kind"] != L.BATCH_NONE:
        outs["feature_matrix"] = (f32, (B, N, N, 1)) if kinds["edge_kind"] == L.BATCH_F32 else (i32, (B, N, N))
    if pe_tail is not None:
        outs["pe"] = (f32, (B, N) + pe_tail)
    outs = {k: v for k, v in outs.items() if k not in null}
    bufs = [Buf("s." + f, IN, t) for f, t in store.items()] + [Buf("idx", IN, torch.tensor(ids, dtype=i32))]
    bufs += [Buf(k, OUT, dtype=dt, shape=shape, graphs=B) for k, (dt, shape) in outs.items()]

    def step(v):
        st = M._struct(L.BatchStore, L.BATCH_STORE_FIELDS, v, "s.")
        ot = L.params_struct(L.BatchOut, L.BATCH_OUT_FIELDS, [v.get(f) for f in L.BATCH_OUT_FIELDS])
        return lib.egt_batch_assemble(C.byref(desc), C.byref(st), M._ptr(v, "idx"), C.byref(ot), M._stream())

    def wrapper(dev):
        return assemble_batch(desc, {f: t.to(dev) for f, t in store.items()}, torch.tensor(ids, dtype=i32, device=dev), list(outs))
    return Case(f"batch_{cid}", bufs, [step], desc=desc, wrapper=wrapper, supported=lambda: lib.egt_batch_supported(C.byref(desc)),
                outputs=sorted(outs))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_batch_assemble_contract(cid, tmp_path, gpu, egt_lib):
    from egt_amd import _lib as L
    case = batch_case(egt_lib, cid, tmp_path)
    assert case.claims["supported"]() == 1
    assert not M.tagged(case), "no parameters or gradient sinks: the store and the outputs keep the allocator's alignment"
    assert set(case.claims["outputs"]) == set(L.BATCH_OUT_FIELDS) - set(CASES[cid][3]) - (
        {"feature_matrix"} if CASES[cid][0].startswith("sbm") else set()) - ({"pe"} if CASES[cid][1] == "matrix" else set())
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)          # runs Z (0x00) and P (0xFF): guards, const inputs, Z == P
    ref = case.claims["wrapper"](gpu)
    assert set(ref) == set(z)
    for name, r in ref.items():
        got = z[name]
        assert r.shape == got.shape and r.dtype == got.dtype, name
        assert torch.equal(got.view(torch.int32), r.contiguous().view(torch.int32)), f"{name}: differs from the Python wrapper's result"
