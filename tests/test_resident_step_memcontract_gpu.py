"""The buffer contract of include/egt_amd.h for the two entries of the resident step, through the harness of
tests/memcontract.py: every buffer in a guarded arena of exactly its byte count, outputs prefilled with 0x00 and with 0xFF.
egt_batch_assemble_at: the cases of tests/test_device_data_memcontract_gpu.py (same stores, same NULL outputs) with the indices
somewhere inside a longer table; the table and the cursor are const inputs, and run Z equals egt_batch_assemble's result.
egt_accumulate: acc is exactly 2K doubles between its guards, the items and the values they point to are const."""
import ctypes as C

import pytest
import torch

import memcontract as M
import test_device_data_memcontract_gpu as BM
from memcontract import Buf, Case, CARRIED, IN, INOUT, OUT

pytestmark = pytest.mark.gpu
PAD = (9, 2, 11)            # table entries in front of the batch's indices: the cursor's value


def at_case(lib, cid, tmp_path):
    from egt_amd import _lib as L
    base = BM.batch_case(lib, cid, tmp_path)
    ids = BM.CASES[cid][2]
    table = torch.tensor(list(PAD) + list(ids) + [0, 5], dtype=torch.int32)
    bufs = [b for b in base.bufs if b.name != "idx"] + [Buf("table", IN, table), Buf("cursor", IN, torch.tensor([len(PAD)], dtype=torch.int64))]
    desc = base.claims["desc"]

    def step(v):
        st = M._struct(L.BatchStore, L.BATCH_STORE_FIELDS, v, "s.")
        ot = L.params_struct(L.BatchOut, L.BATCH_OUT_FIELDS, [v.get(f) for f in L.BATCH_OUT_FIELDS])
        return lib.egt_batch_assemble_at(C.byref(desc), C.byref(st), M._ptr(v, "table"), M._ptr(v, "cursor"), C.byref(ot), M._stream())
    return Case(f"batch_at_{cid}", bufs, [step], **base.claims)


@pytest.mark.parametrize("cid", sorted(BM.CASES))
def test_batch_assemble_at_contract(cid, tmp_path, gpu, egt_lib):
    from egt_amd import _lib as L
    case = at_case(egt_lib, cid, tmp_path)
    assert case.claims["supported"]() == 1 and not M.tagged(case)
    null = set(BM.CASES[cid][3])
    assert null.isdisjoint(b.name for b in case.bufs) and {b.name for b in case.bufs if b.role == OUT} == set(case.claims["outputs"])
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)      # runs Z and P: guards, const table / cursor / store, Z == P
    ref = case.claims["wrapper"](gpu)                                          # egt_batch_assemble on the batch's own indices
    assert set(ref) == set(z)
    for name, r in ref.items():
        assert torch.equal(z[name].view(torch.int32), r.contiguous().view(torch.int32)), name


def accumulate_case(lib, K, with_count):
    from egt_amd import _lib as L
    gen = torch.Generator().manual_seed(K)
    vals = torch.randn(2 * K, generator=gen) * 1e3
    acc0 = torch.randn(2 * K, generator=gen, dtype=torch.float64)
    bufs = [Buf("acc", INOUT, acc0), Buf("vals", IN, vals), Buf("items", CARRIED, nbytes=C.sizeof(L.AccItem) * K, const_after=0, compare=False)]

    def fill_items(v):                      # the item table names addresses inside this run's arenas: written by the host, then const
        items = (L.AccItem * K)()
        for k in range(K):
            items[k].sum = v["vals"].data_ptr() + 8 * k
            items[k].count = v["vals"].data_ptr() + 8 * k + 4 if with_count[k] else None
            items[k].count_value = 0.0 if with_count[k] else 3.0 + k
        v["items"].copy_(torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8))
        return L.EGT_OK

    def step(v):
        return lib.egt_accumulate(M._ptr(v, "acc"), M._ptr(v, "items"), K, M._stream())
    want = acc0.clone()
    for _ in range(2):
        for k in range(K):
            want[2 * k] += float(vals[2 * k])
            want[2 * k + 1] += float(vals[2 * k + 1]) if with_count[k] else 3.0 + k
    return Case(f"accumulate_k{K}", bufs, [fill_items, step, step], want=want)


@pytest.mark.parametrize("K,with_count", [(1, (False,)), (3, (True, False, True)), (32, tuple(k % 3 != 1 for k in range(32)))])
def test_accumulate_contract(K, with_count, gpu, egt_lib):
    from egt_amd import _lib as L
    case = accumulate_case(egt_lib, K, with_count)
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    assert torch.equal(z["acc"].cpu(), case.claims["want"]), "two launches: the host's two rounds of fp64 additions, NULL counts by their constant"
