"""egt_block_plan_static without a GPU: which descriptors plan_block gives the compile-time forward instance (k_block_fwd_s64).  The plan
switches are read once per process, so each environment is a fresh child process (tests/test_headline_static_gpu.py in its plan-only
mode: no device work; egt_device_cus() answers 256 without a device, the MI355X's count)."""
import os
import tempfile

import test_headline_static_gpu as T


def _plan(env):
    with tempfile.TemporaryDirectory() as tmp:
        return T._child(tmp, env, run=False)


def test_plan_static_with_the_row_overrides(egt_lib):
    out = _plan(T.ROW_ENV)
    assert out["plan"] == dict(headline=1, n48=0, no_clip=0, prob0=0, null=0)
    assert out["form"] == "fwd=k_block_fwd/4w bwd=k_block_bwd_v5/4w/tl16"


def test_no_static_switch_clears_the_plan_bit(egt_lib):
    out = _plan(dict(T.ROW_ENV, EGT_NO_STATIC="1"))
    assert set(out["plan"].values()) == {0}
    assert out["form"] == "fwd=k_block_fwd/4w bwd=k_block_bwd_v5/4w/tl16"      # the launch form itself does not move


def test_small_batch_plans_short_row_groups_and_the_generic_instance(egt_lib):
    out = _plan({})
    assert set(out["plan"].values()) == {0} and "tl16" not in out["form"]


def test_headline_batch_plans_the_static_instance_in_this_process(egt_lib):
    """B = 128 needs no override: 16-row groups are the plan (this process's environment, unless it sets a plan switch itself)"""
    import ctypes as C
    from egt_amd import _lib as L
    if any(os.environ.get(k) for k in ("EGT_NO_STATIC", "EGT_FWD_ROWS")):
        return
    d = T.make_desc(L)
    d.B = 128
    assert egt_lib.egt_block_plan_static(C.byref(d)) == 1
    d.dtype = L.EGT_BF16
    assert egt_lib.egt_block_plan_static(C.byref(d)) == 0
    d.dtype, d.flags = L.EGT_F32, d.flags | L.BF_ATTN_MASK
    assert egt_lib.egt_block_plan_static(C.byref(d)) == 0
