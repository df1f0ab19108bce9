"""The buffer contract of include/egt_amd.h for egt_attn_mfma_fwd / egt_attn_mfma_bwd with EGT_ATTN_MM_BF16, in the guarded arenas
of tests/memcontract.py (the table's own MFMA cases with the bit added to their descriptor): no write outside the declared
outputs and the workspace, const inputs untouched, results independent of what outputs and workspace held before (0x00 and 0xFF
prefill: bit-equal), with the shared and the per-call workspace.  So that a case cannot be bit-stable and wrong, run Z is held to
the plain fp64 oracle at BF16_TOL (the tight bounds of the mode are tests/test_attn_bf16_gpu.py's)."""
import ctypes as C

import pytest
import torch

import memcontract as M
from attn_bf16_ref import BF16_TOL
from util import assert_close

pytestmark = pytest.mark.gpu
SHAPES = [(2, 21, 32), (1, 17, 64)]


def _lib():
    from egt_amd import build, _lib as L
    build.build()
    return L.load()


def _cases():
    from egt_amd import _lib as L
    lib, out = _lib(), []
    for B, N, d in SHAPES:
        for shared in (False, True):
            c = M.mfma_case(lib, B, N, d, shared)
            desc = c.claims["desc"]
            desc.reserved |= L.ATTN_MM_BF16                    # the steps' descriptor (they hold a reference to it)
            query = {"ws": lib.egt_attn_mfma_workspace_bytes, "ws_fwd": lib.egt_attn_mfma_fwd_workspace_bytes}
            # the workspace arenas get EXACTLY what the size queries answer for the bit (smaller than the table's: bf16 dA tiles)
            c.bufs = [M.Buf(b.name, b.role, nbytes=query[b.name](C.byref(desc)), graphs=b.graphs) if b.name in query else b for b in c.bufs]
            c.name = c.name.replace("mfma_", "mfma_bf16_")
            out.append(pytest.param(c, id=c.name))
    return out


@pytest.mark.parametrize("case", _cases())
def test_attn_bf16_contract(case, gpu, egt_lib):
    from egt_amd import _lib as L
    desc = case.claims["desc"]
    assert desc.reserved & L.ATTN_MM_BF16 and egt_lib.egt_attn_mfma_supported(C.byref(desc), 0) == 1
    sizes = {b.name: b.nbytes for b in case.bufs if b.name.startswith("ws")}
    assert sizes["ws"] == egt_lib.egt_attn_mfma_workspace_bytes(C.byref(desc))             # the arenas have the sizes the bit asks for
    if "ws_fwd" in sizes:
        assert sizes["ws_fwd"] == egt_lib.egt_attn_mfma_fwd_workspace_bytes(C.byref(desc))
    z = M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    for name, (ref, _) in case.claims["oracle"]().items():
        if name in z:
            assert_close(z[name].float(), ref, name=f"{case.name}:{name} vs the fp64 oracle", **BF16_TOL)
