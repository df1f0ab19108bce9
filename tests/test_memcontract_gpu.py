"""The buffer contract of include/egt_amd.h ("Buffer contract"), entry point by entry point, through the C ABI itself (the
Python wrappers allocate their own buffers, which cannot be guarded).  tests/memcontract.py holds the harness and the case
table: every tensor of a call sits in a guarded arena of exactly the stated byte count, and each case runs with outputs /
scratch prefilled with 0x00 (run Z), with 0xFF (run P: NaN as fp32 and bf16) and once per allowed aliasing (run A).  Parameter
tensors and gradient sinks are held to element alignment only: three more poisoned runs put them 4, 8 or 12 bytes past the
512-byte boundary (U-sinks: the sinks, as FlatGradAllReduce(direct=True) lays them out; U-all: parameters too; U-mixed: half of
each, so one call sees both kinds).  Asserted: guards untouched, const inputs untouched, runs P and U finite, Z == P == A == U
bit for bit.  So that a case cannot be bit-stable and wrong,
run Z is also held to the fp64 oracle (inner op, block, stack, FFN: the suite's FWD / BWD tolerances; bf16 storage: the suite's
bf16_stack_tol) or, where tests/cases.py has no oracle, to the Python wrapper's result on the same inputs, bit for bit (the
parity tests tie that result to the oracle).

Exclusions from "fully written / prefill-independent" (each names its header sentence in the case):
  * egt_attn_fwd's rowstats slot 3: "rowstats [B,N,H,4] fp32 (softmax max, softmax sum, gate degree, reserved)".
The EGT_BF_NO_EDGE_LN "gradient outputs are scratch" pointers do not occur: the table's 'bias' cases carry EGT_BF_STATIC_EDGE,
where those pointers are NULL.

The block and stack tables run again in two child processes (the plan's switches are read once per process): the full-size
launch geometry (EGT_BWD_TL=16 EGT_FWD_ROWS=16: dkvp / epart sizes follow nwg_bwd) and EGT_NO_NARROW=1 (De = 8 on r4 / v4r;
without the static-edge cases, which block_check refuses there).  Of the U runs the children make U-all."""
import os
import subprocess
import sys

import pytest
import torch

import memcontract as M
from util import assert_close, bf16_stack_tol, FWD, BWD

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "EGT_MEMCONTRACT_CHILD"
NO_NARROW = os.environ.get("EGT_NO_NARROW", "") not in ("", "0")


def _lib():
    from egt_amd import build, _lib as L
    build.build()                       # (as the egt_lib fixture: the cases are built at collection, from the size queries)
    return L.load()


def _cases(family, **kw):
    """the family's cases, built once at collection (size queries only: no GPU is touched)"""
    return [pytest.param(c, id=c.name) for c in M.FAMILIES[family](_lib(), **kw)]


def _check(case, gpu):
    from egt_amd import _lib as L
    sup = case.claims.get("supported")
    assert sup is None or sup() == 1, f"{case.name}: the library does not cover the case"
    return M.check(case, gpu, sync=torch.cuda.synchronize, check_rc=L.check, u_runs=("all",) if os.environ.get(CHILD) else M.U_RUNS)


def _hold_to_oracle(case, z, layers=1):
    bf16 = bool(case.claims.get("bf16") or (case.claims.get("row") and case.claims["row"][5]))
    for name, (ref, is_grad) in case.claims["oracle"]().items() if "oracle" in case.claims else M.block_oracle(case).items():
        if name == "a_tild" and "a_tild" not in z:          # the oracle always has it; the case did not ask for it
            continue
        assert name in z, f"{case.name}: the oracle's '{name}' matches no compared buffer of the case"
        got = z[name]
        if got.dtype == torch.bfloat16 or (bf16 and "row" in case.claims):     # bf16 storage (a stack also rounds e_l between layers)
            tol = dict(bf16_stack_tol(layers, params=name.startswith("g")), zero_atol=2e-4)
        else:
            tol = BWD if is_grad else FWD
        assert_close(got.float(), ref, name=f"{case.name}:{name} vs the fp64 oracle", **tol)


def _hold_to_wrapper(case, z, gpu):
    for name, ref in case.claims["wrapper"](gpu).items():
        got = z[name]
        assert ref.shape == got.shape and ref.dtype == got.dtype, f"{case.name}:{name}"
        itype = M._ITYPE[got.element_size()]
        same = got.contiguous().view(itype) == ref.contiguous().view(itype)
        assert bool(same.all()), f"{case.name}:{name}: {int((~same).sum())}/{got.numel()} elements differ from the Python wrapper's result"


# what the switches of the two child runs must have done to the plan of the De = 8 row "n19_de8" (CHILD names the run)
CHILD_FORMS = {"full-size": ("k_narrow_fwd/4w", "k_narrow_bwd/4w/tl16"), "no-narrow": ("k_block_fwd_r4/4w", "k_block_bwd_v4r/4w/tl8")}


def test_child_run_switches_moved_the_plan(egt_lib):
    """In a child run: the environment reached the library's plan (a renamed switch would make the run a duplicate of the first).
    In the parent: the default plan, as tests/test_memcontract_cpu.py pins it."""
    import ctypes as C
    row = M.BLOCK_TABLE[0]
    assert row[0] == "n19_de8"
    desc = M.block_desc(row)
    form = egt_lib.egt_block_launch_form(C.byref(desc)).decode()
    want = CHILD_FORMS[os.environ[CHILD]] if os.environ.get(CHILD) else (row[7], row[8])
    assert form == f"fwd={want[0]} bwd={want[1]}"


@pytest.mark.parametrize("case", _cases("block", static=not NO_NARROW))
def test_block_contract(case, gpu, egt_lib):
    z = _check(case, gpu)
    _hold_to_oracle(case, z)
    if "static" in case.claims["row"][6]:
        assert "e_out" not in z            # (handed over as a const buffer: "e_out is never written" was held by the runner)


@pytest.mark.parametrize("case", _cases("stack"))
def test_stack_contract(case, gpu, egt_lib):
    z = _check(case, gpu)
    _hold_to_oracle(case, z, layers=case.claims["layers"])


def _child(which, env_extra):
    env = dict(os.environ, **env_extra)
    env[CHILD] = which
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    here = "tests/" + os.path.basename(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        f"{here}::test_child_run_switches_moved_the_plan", f"{here}::test_block_contract", f"{here}::test_stack_contract"], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert " passed" in r.stdout


if not os.environ.get(CHILD):
    def test_block_and_stack_again_in_the_full_size_launch_geometry():
        _child("full-size", {"EGT_BWD_TL": "16", "EGT_FWD_ROWS": "16"})

    def test_block_and_stack_again_on_the_mfma_tile_kernels_at_de8():
        _child("no-narrow", {"EGT_NO_NARROW": "1"})


@pytest.mark.parametrize("case", _cases("attn"))
def test_attn_contract(case, gpu, egt_lib):
    _hold_to_oracle(case, _check(case, gpu))


@pytest.mark.parametrize("case", _cases("mfma"))
def test_attn_mfma_contract(case, gpu, egt_lib):
    _hold_to_oracle(case, _check(case, gpu))


@pytest.mark.parametrize("case", _cases("pair"))
def test_pair_contract(case, gpu, egt_lib):
    _hold_to_wrapper(case, _check(case, gpu), gpu)


@pytest.mark.parametrize("case", _cases("edge"))
def test_edge_ops_contract(case, gpu, egt_lib):
    _hold_to_wrapper(case, _check(case, gpu), gpu)


@pytest.mark.parametrize("case", _cases("ffn"))
def test_ffn_contract(case, gpu, egt_lib):
    _hold_to_oracle(case, _check(case, gpu))


@pytest.mark.parametrize("case", _cases("embed"))
def test_edge_embed_contract(case, gpu, egt_lib):
    _hold_to_wrapper(case, _check(case, gpu), gpu)


@pytest.mark.parametrize("case", _cases("head"))
def test_heads_contract(case, gpu, egt_lib):
    z = _check(case, gpu)
    _hold_to_wrapper(case, z, gpu)
    if "mask" in case.claims:            # "d_h gets exact zeros on masked rows" (Z == P: in the poisoned run too)
        masked = z["d_h"][case.claims["mask"].to(gpu) == 0]
        assert masked.numel() > 0 and bool((masked.view(torch.int32) == 0).all())


@pytest.mark.parametrize("case", _cases("mask"))
def test_mask_producers_contract(case, gpu, egt_lib):
    z = _check(case, gpu)
    if "words" in case.claims:
        want = (case.claims["words"] + torch.tensor(0xD1B54A32D192ED03 - (1 << 64), dtype=torch.int64))
        assert torch.equal(z["words"].cpu(), want)
