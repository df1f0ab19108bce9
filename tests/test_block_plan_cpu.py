"""The fused block's launch plan (egt_block.hip: plan_block) pinned without a GPU: for the bench workloads' shapes, every edge
width with and without an attention mask, and small N, the backward kernel family (egt_block_bwd_kernel) and the buffer sizes
(the workspace encodes the backward's rows per workgroup) against tests/golden/block_plan.json.  The plan's switches are read
once per process, so each setting runs in a child process: `python tests/test_block_plan_cpu.py` prints the table of the
current environment (how the golden file was recorded, one entry per setting).  The shape rules assume 256 CUs: the MI355X
and the no-GPU fallback of egt_device_cus() both give that."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "block_plan.json")
SETTINGS = {"default": {}, "EGT_BWD_TL=5": {"EGT_BWD_TL": "5"}, "EGT_NO_NARROW_BWD=1": {"EGT_NO_NARROW_BWD": "1"}}


def cases():
    """(name, B, N, d, De, bf16, attn_mask)"""
    out = [("zinc500k_n64", 128, 64, 8, 64, False, False),
           ("zinc100k_n37", 128, 37, 6, 48, False, False),
           ("cifar10_n150", 128, 150, 8, 8, True, False),
           ("cifar10_n150_fp32", 128, 150, 8, 8, False, False),
           ("pattern500k_n120", 16, 120, 8, 8, False, False),
           ("pattern500k_n120_b128", 128, 120, 8, 8, False, False),
           ("pattern500k_n188", 16, 188, 8, 8, False, False)]
    for De in (8, 16, 32, 48, 64):
        for bf in ((False, True) if De >= 32 else (False,)):
            for ml in (False, True):
                for B, N in ((16, 120), (128, 64), (32, 50)):
                    out.append((f"De{De}_{'bf16' if bf else 'fp32'}{'_mask' if ml else ''}_B{B}_N{N}", B, N, 8, De, bf, ml))
    for N in (6, 9, 37):
        for B in (1, 128):
            for De in (8, 64):
                out.append((f"small_N{N}_B{B}_De{De}", B, N, 8, De, False, False))
    return out


def table(lib):
    from egt_amd import _lib as L
    rows = {}
    for name, B, N, d, De, bf, ml in cases():
        flags = L.BF_GATE | L.BF_CLIP | L.BF_TRAINING | (L.BF_ATTN_MASK if ml else 0)
        desc = L.BlockDesc(B=B, N=N, H=8, d=d, De=De, dtype=L.EGT_BF16 if bf else L.EGT_F32, flags=flags, clip_lo=-5.0,
                           clip_hi=5.0, random_mask_prob=0.1, ln_eps=1e-5, reserved=0, seed=0, seed_device=None)
        p = C.byref(desc)
        kernel = lib.egt_block_bwd_kernel(p)
        rows[name] = [kernel.decode() if kernel else None, lib.egt_block_workspace_bytes(p), lib.egt_block_saved_bytes(p),
                      lib.egt_stack_workspace_bytes(p, 4), lib.egt_stack_saved_bytes(p, 4)]
    return rows


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_block_plan_matches_golden(egt_lib, setting):
    env = dict(os.environ)
    for k in ("EGT_NO_NARROW", "EGT_NO_NARROW_FWD", "EGT_NO_NARROW_BWD", "EGT_BWD_MATMUL", "EGT_BWD_TL", "EGT_FWD_ROWS",
              "EGT_NRW_FWD_WAVES", "EGT_NRW_FWD_HALF", "EGT_NRW_BWD_WAVES"):
        env.pop(k, None)
    env.update(SETTINGS[setting])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = json.load(open(GOLDEN))[setting]
    assert set(got) == set(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"[kernel, block ws, block saved, stack ws (4), stack saved (4)]: got vs golden {bad}"


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from egt_amd import _lib
    print(json.dumps(table(_lib.load()), sort_keys=True))
