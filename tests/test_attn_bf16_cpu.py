"""The bf16-product mode of the MFMA inner op (EGT_ATTN_MM_BF16, AttnConfig(matmul="bf16")) without a GPU: the flag in the header
and its Python mirror, the workspace sizes for the bit against tests/golden/attn_bf16_workspace.json (recorded by
`python tests/test_attn_bf16_cpu.py`, like op_workspace.json), the validation of the three front-ends, the block's route, and the
fairness cap of ATTN_BF16_TOL: the contract alone (fp64 emulation of its six roundings against the oracle fed the rounded
operands) uses at most half of it on every case the GPU tests run."""
import ctypes as C
import json
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "attn_bf16_workspace.json")


def test_flag_in_header_and_mirror():
    from egt_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    val = lambda name: int(re.search(rf"#define {name} (0x[0-9a-fA-F]+)", hdr).group(1), 16)
    assert val("EGT_ATTN_MM_BF16") == 0x2 == L.ATTN_MM_BF16
    assert val("EGT_ATTN_WS_SHARED") == L.ATTN_WS_SHARED
    assert L.ATTN_MM_BF16 & L.ATTN_WS_SHARED == 0


def table(lib):
    """the grid of tests/test_op_workspace_cpu.py: name -> ([both, forward alone, forward shared] with the bit, the same without)"""
    from egt_amd import _lib as L
    rows = {}
    flags = L.F_EDGE_INPUT | L.F_GATE_INPUT | L.F_CLIP | L.F_TRAINING
    for d in (16, 32, 64, 24):
        for N in (1, 15, 16, 37, 512, 2048, 2049):
            for B in (1, 8, 32):
                got = {}
                for mm in (L.ATTN_MM_BF16, 0):
                    q = []
                    for ws in (0, L.ATTN_WS_SHARED):
                        desc = L.AttnDesc(B=B, N=N, H=8, d=d, dtype=L.EGT_F32, flags=flags, clip_lo=-5.0, clip_hi=5.0,
                                          random_mask_prob=0.1, attn_dropout=0.0, num_virtual_nodes=0, reserved=ws | mm, seed=0)
                        if not ws:
                            q.append(lib.egt_attn_mfma_workspace_bytes(C.byref(desc)))
                        q.append(lib.egt_attn_mfma_fwd_workspace_bytes(C.byref(desc)))
                    got[mm] = q
                rows[f"attn_bf16_d{d}_N{N}_B{B}"] = (got[L.ATTN_MM_BF16], got[0])
    return rows


def test_workspace_sizes_for_the_bit(egt_lib):
    rows = table(egt_lib)
    want = json.load(open(GOLDEN))
    assert set(rows) == set(want)
    for name, (bf, f32) in rows.items():
        both, fwd, shared = bf
        if f32[0] == 0:
            assert bf == [0, 0, 0], name                    # 0 exactly where the fp32 query is 0
            continue
        assert 0 < both <= f32[0] and 0 < fwd <= f32[1], name
        assert fwd <= both and shared == both, name
        assert bf == want[name], f"{name}: got {bf}, golden {want[name]}"
    assert any(f32[0] == 0 for _, f32 in rows.values()) and any(f32[0] > 0 for _, f32 in rows.values())


def test_front_end_validation():
    from egt_amd import AttnConfig, EGT
    from egt_amd.layers import EGTBlock
    assert AttnConfig().matmul == "f32" and AttnConfig(matmul="bf16").matmul == "bf16"
    for bad in ("fp16", "bf16x3", "", None):
        with pytest.raises(ValueError):
            AttnConfig(matmul=bad)
        with pytest.raises(ValueError):
            EGT(matmul=bad)
        with pytest.raises(ValueError):
            EGTBlock(model_width=128, edge_width=32, attn_matmul=bad)
    assert EGT().matmul == "f32" and EGT(matmul="bf16").matmul == "bf16"
    blk = EGTBlock(model_width=128, edge_width=32, attn_matmul="bf16")
    assert blk.attn_matmul == "bf16" and blk.mha.matmul == "bf16"
    assert EGTBlock(model_width=128, edge_width=32).mha.matmul == "f32"
    for width in (64, 48, 1024, 192):                        # head dims 8, 6, 128, 24: not on the MFMA inner op
        with pytest.raises(ValueError, match="16, 32, 64"):
            EGTBlock(model_width=width, edge_width=32, attn_matmul="bf16")
    for width in (128, 256, 512):
        EGTBlock(model_width=width, edge_width=32, attn_matmul="bf16")
    with pytest.raises(ValueError):
        EGTBlock(model_width=128, edge_width=32, attn_matmul="bf16", scale_degree=True)
    with pytest.raises(ValueError):
        EGTBlock(model_width=128, edge_width=32, attn_matmul="bf16", attn_dropout=0.1)
    with pytest.raises(ValueError):
        EGTBlock(model_width=512, edge_width=32, attn_matmul="bf16", fused=True)


def test_block_route(egt_lib):
    """width 512 / De 32 (d = 64): the default takes the pair operator, attn_matmul='bf16' the composed operator (the pair
    operator has no such mode); the d = 16 block is composed either way"""
    from egt_amd import fused as FZ
    from egt_amd.layers import EGTBlock
    for train in (False, True):
        args = (2, 16, torch.float32, torch.float32, True)
        blk = EGTBlock(model_width=512, edge_width=32).train(train)
        assert FZ.route_core(blk, *args) == ("fused-pair", None)
        blk = EGTBlock(model_width=512, edge_width=32, attn_matmul="bf16").train(train)
        assert FZ.route_core(blk, *args) == ("composed", None)
        blk = EGTBlock(model_width=128, edge_width=32, attn_matmul="bf16").train(train)
        assert FZ.route_core(blk, *args) == ("composed", None)


def _cpu_case(name):
    import attn_bf16_ref as R
    from oracle import rng_ref
    if name in R.CASES:
        return R.make_case(name) + (R.CASES[name][2],)
    B, N, d = R.RNG_CASES[name]
    rm = torch.from_numpy(rng_ref.random_mask(R.RNG_SEED, B, N, R.H, R.RNG_P))
    return R.make_rng_case(name, rm) + (d,)


def _all_cases():
    import attn_bf16_ref as R
    return list(R.CASES) + list(R.RNG_CASES)


@pytest.mark.parametrize("name", ["n21_d32", "n24_d16_attn_mask", "n21_d32_ungated", "n33_d64_noclip_nomask", "n16_d16_randmask"])
def test_emulation_without_rounding_is_the_oracle(name):
    """the hand-written forward / backward of the emulation, roundings off, against the autograd oracle: fp64 noise only"""
    import attn_bf16_ref as R
    import cases as CS
    inp, attrs, d = _cpu_case(name)
    ref = CS.attn_oracle(inp, attrs)
    got = R.emulate(inp, attrs, d, round=False)
    for k, v in got.items():
        if v is None:
            assert ref[k] is None
        else:
            assert float((v - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), k


@pytest.mark.parametrize("name", _all_cases())
def test_fairness_cap(name):
    """the contract alone stays within half of ATTN_BF16_TOL (elementwise and L2) against the oracle fed the rounded operands;
    H_hat and dG carry no bf16 error at all.  Measured worst: 0.38 elementwise (dQKV, n48_d64), 0.34 of the L2 bound."""
    import attn_bf16_ref as R
    from util import margin
    inp, attrs, d = _cpu_case(name)
    ref = R.oracle_rounded(inp, attrs, d)
    got = R.emulate(inp, attrs, d)
    for k in ("H_hat", "dG"):
        if got[k] is not None:
            assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), k
    for k in ("V_att", "dQKV", "dE"):
        if got[k] is None:
            continue
        m = margin(got[k], ref[k], rtol=R.ATTN_BF16_TOL["rtol"], arel=R.ATTN_BF16_TOL["arel"])
        l2 = float((got[k] - ref[k]).norm() / ref[k].norm())
        print(f"[attn_bf16 fairness] {name} {k}: elementwise {m:.3f}, L2 {l2 / R.ATTN_BF16_TOL['l2']:.3f} of ATTN_BF16_TOL")
        assert m <= 0.5, (k, m)
        assert l2 <= 0.5 * R.ATTN_BF16_TOL["l2"], (k, l2)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from egt_amd import _lib
    rows = {k: v[0] for k, v in table(_lib.load()).items()}
    print("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(rows[k])}" for k in sorted(rows)) + "\n}")
