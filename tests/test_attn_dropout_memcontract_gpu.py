"""Memory contract of egt_block_fwd / egt_block_bwd with EGT_BF_ATTN_DROPOUT: two rows of the existing block table
(tests/memcontract.py, imported as it is) with the flag and the rate set on their descriptors -- guarded arenas, the Z / P / U runs,
and run Z held to the fp64 oracle with the keep mask of the descriptor's seed.  The flagged descriptor asks for the same `saved`
and workspace bytes as the unflagged one (nothing is stored for the mask), so the table's buffers are the flagged call's."""
import ctypes as C

import pytest
import torch

import memcontract as M
from util import assert_close, FWD, BWD

pytestmark = pytest.mark.gpu
ROWS = {r[0]: r for r in M.BLOCK_TABLE}
RATE = 0.25
CASES = [("n19_de64", "k_block_bwd_v5"), ("n21_de16", "k_block_bwd_v4r")]


def _oracle(case):
    from oracle import egt_oracle as O, rng_ref
    row, inp = case.claims["row"], case.claims["inp"]
    _, B, N, d, De, _, _, _, _ = row
    rm = torch.from_numpy(rng_ref.random_mask(M.SEED, B, N, 8, M.RAND_P))
    keep = torch.from_numpy(rng_ref.dropout_keep(M.SEED, B, N, 8, RATE))
    h = inp["h"].double().requires_grad_(); e = inp["e"].double().requires_grad_()
    p = {k: t.double().requires_grad_() for k, t in zip(M.BLOCK_ORACLE_NAMES, inp["params"][0])}
    h2, e2 = O.block_forward(h, e, inp["key_mask"].bool(), p, num_heads=8, rand_mask=rm, drop_keep=keep, attn_dropout=RATE)
    loss = (h2 * inp["dh"].double()).sum() + (e2 * inp["de"].double()).sum()
    gr = torch.autograd.grad(loss, [h, e] + list(p.values()))
    from egt_amd import _lib as L
    out = {"h_out": (h2.detach(), False), "e_out": (e2.detach(), False), "d_h": (gr[0], True), "d_e": (gr[1], True)}
    out.update({f"g0.{f}": (g, True) for f, g in zip(L.BLOCK_PARAM_FIELDS, gr[2:])})
    return out


@pytest.mark.parametrize("name,bwd", CASES)
def test_flagged_block_contract(name, bwd, gpu, egt_lib):
    from egt_amd import _lib as L
    case = M.block_case(egt_lib, ROWS[name])
    desc = case.claims["desc"]
    p = C.byref(desc)
    sizes = egt_lib.egt_block_saved_bytes(p), egt_lib.egt_block_workspace_bytes(p)
    desc.flags |= L.BF_ATTN_DROPOUT                      # (the case's calls hold this descriptor; EGT_BF_TRAINING is the table's)
    desc.reserved = L.rate_bits(RATE)
    assert egt_lib.egt_block_supported(p) == 1
    assert (egt_lib.egt_block_saved_bytes(p), egt_lib.egt_block_workspace_bytes(p)) == sizes
    assert egt_lib.egt_block_bwd_kernel(p).decode() == bwd
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    for k, (ref, is_grad) in _oracle(case).items():
        assert_close(z[k].float(), ref, name=f"{name}:{k} vs the fp64 oracle", **(BWD if is_grad else FWD))
