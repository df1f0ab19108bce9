"""GPU parity of egt_stack_bwd's closing kernels -- k_node_wgrads, k_sum_segments, k_edge_param_grads -- across their launch
plane, against the fp64 oracle.  tests/stack_tail.py holds the shape table (one row per class of the plane: the five- and six-step
walks of k_node_wgrads with ragged last chunks, at Dh = 64 and below; every path of k_sum_segments; the 11-layer and 16-layer
launch cuts; the three ways the forward prepares the edge weights; 64 layers), the seeded recipe and the cached oracle;
tests/test_stack_tail_cpu.py holds the table to the library's own plan and the comparison to fairness.

One id per row: EGTStack(fused=True) forward and backward in one call under the launch profiler; h', e' at the tolerance of
test_stack_call_vs_oracle, dh, de and EVERY parameter gradient of EVERY layer under util.BWD, failures reported by layer and
parameter; the launch counts plan_tail() predicts; a second run bit-identical.  Two rows run again through the C ABI in the guarded
arenas of tests/memcontract.py: buffers of exactly the queried sizes, prefilled with 0x00 (run Z) and 0xFF (run P) -- a reduction
that reads a partial slot nobody wrote shows as NaN in run P or as a difference between the two.

Mutants this file was checked against (scratch builds, never committed; ids are rows of the table):
  (a) k_node_wgrads ends its walk at rbeg + WG_ROWS: fails b128_n33_de8_dh64_ly16, b36_n30_de64_dh64_ly58,
      b44_n30_de16_dh64_ly64 and b50_n31_de48_dh48_ly40 (the rows above 128 rows per workgroup) on dense_qkv.kernel /
      dense_mha.kernel only, passes the other three;
  (b) k_sum_segments drops the partial round after a full one: fails b36_n30_de64_dh64_ly58, b44_n30_de16_dh64_ly64 and
      b50_n31_de48_dh48_ly40 (the 'full+partial' rows) on every gradient reduced over the backward's workgroups and on neither
      weight gradient; passes the 'full' row and the 'mixed' one, where no lane group runs both rounds.
The memory-contract ids pass under both (they compare two runs of one build)."""
import pytest
import torch

import memcontract as M
import stack_tail as ST
from util import BWD, assert_close

pytestmark = pytest.mark.gpu


def _failures(got, ref):
    """[message] of every tensor out of tolerance, named by layer and parameter"""
    bad = []
    for (name, a, is_grad), (_, r, _) in zip(ST.tensors(got), ST.tensors(ref)):
        try:
            assert_close(a, r, name=name, **(BWD if is_grad else ST.FWD_TOL))
        except AssertionError as err:
            bad.append(str(err))
    return bad


@pytest.mark.parametrize("row", list(ST.ROWS), ids=ST.row_id)
def test_stack_tail_vs_oracle(row, gpu, egt_lib):
    p = ST.plan_tail(*row)
    tail, bwd = ST.library_forms(egt_lib, row)
    assert (tail, bwd) == (p["tail_form"], p["bwd_form"]), "this device's plan is not the table's (another CU count?)"
    st = ST.build_stack(row, gpu)
    got, count = ST.launch_counts(egt_lib, lambda: ST.run_gpu(st, row, gpu))
    ref = ST.oracle(row)
    m = ST.margins(got, ref)
    worst = max(m, key=m.get)
    print(f"{ST.row_id(row)}: {tail}; worst margin {m[worst]:.3f} ({worst}); "
          f"weight gradients {max(v for k, v in m.items() if k.endswith(ST.WGRAD_PARAMS)):.3f}")
    bad = _failures(got, ref)
    assert not bad, f"{ST.row_id(row)} ({tail}; edge partials '{p['edge_class']}', weight partials '{p['weight_class']}'): " \
                    f"{len(bad)} tensors out of tolerance:\n" + "\n".join(bad[:12])
    Ly = row[4]
    assert count.get("k_node_wgrads") == 1, count
    assert count.get("k_sum_segments") == p["reduce_launches"] == -(-Ly // 11), count
    assert count.get("k_edge_param_grads") == p["epg_launches"] == -(-Ly // 16), count
    assert (count.get("k_edge_prep", 0) > 0) == p["edge_prep"] == (Ly > 40), count
    # fixed association order everywhere in the tail: a second run gives the same bits
    again = ST.run_gpu(st, row, gpu)
    for (name, a, is_grad), (_, b, _) in zip(ST.tensors(got), ST.tensors(again)):
        assert torch.equal(a, b), f"{ST.row_id(row)}: {name} differs between two runs of the same call"


@pytest.mark.parametrize("mrow,layers", M.STACK_TAIL_TABLE, ids=[r[0] for r, _ in M.STACK_TAIL_TABLE])
def test_stack_tail_memory_contract(mrow, layers, gpu, egt_lib):
    from egt_amd import _lib as L
    case = M.stack_case(egt_lib, mrow, layers)
    kw = dict(sync=torch.cuda.synchronize, check_rc=L.check)
    z = M.run(case, M.ZERO, gpu, **kw)            # (run() checks every guard and every const input after each step)
    p = M.run(case, M.POISON, gpu, **kw)
    M.assert_finite(case, p)
    M.assert_same_bits(case, z, p)
    assert sum(1 for b in case.bufs if b.ptr == M.SINK) == 14 * layers
