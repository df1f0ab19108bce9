"""Workspace sizes of the MFMA inner attention, the fused pair operator and the fused FFN pinned without a GPU: every size query
of egt_attn_mfma.hip (plan_attn) and egt_ffn.hip (plan_ffn) over a grid of ragged and unsupported shapes (0 = not covered)
against tests/golden/op_workspace.json.  None of these sizes depends on a switch or on the device, so the table is computed in
process; `python tests/test_op_workspace_cpu.py` prints it (how the golden file was recorded)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "op_workspace.json")


def table(lib):
    from egt_amd import _lib as L
    rows = {}
    attn_flags = L.F_EDGE_INPUT | L.F_GATE_INPUT | L.F_CLIP | L.F_TRAINING
    for d in (16, 32, 64, 24):
        for N in (1, 15, 16, 37, 512, 2048, 2049):
            for B in (1, 8, 32):
                got = []
                for reserved in (0, L.ATTN_WS_SHARED):
                    desc = L.AttnDesc(B=B, N=N, H=8, d=d, dtype=L.EGT_F32, flags=attn_flags, clip_lo=-5.0, clip_hi=5.0,
                                      random_mask_prob=0.1, attn_dropout=0.0, num_virtual_nodes=0, reserved=reserved, seed=0)
                    if not reserved:
                        got.append(lib.egt_attn_mfma_workspace_bytes(C.byref(desc)))
                    got.append(lib.egt_attn_mfma_fwd_workspace_bytes(C.byref(desc)))
                rows[f"attn_d{d}_N{N}_B{B}"] = got   # [both directions, forward alone, forward with EGT_ATTN_WS_SHARED]

    def pair(B, N, d=64, mask=False):
        flags = L.BF_GATE | L.BF_CLIP | L.BF_TRAINING | (L.BF_ATTN_MASK if mask else 0)
        desc = L.BlockDesc(B=B, N=N, H=8, d=d, De=32, dtype=L.EGT_F32, flags=flags, clip_lo=-5.0, clip_hi=5.0,
                           random_mask_prob=0.1, ln_eps=1e-5, reserved=0, seed=0, seed_device=None)
        return lib.egt_pair_workspace_bytes(C.byref(desc))
    for B in (1, 8, 32):
        for N in (1, 17, 512, 2048, 2049):
            rows[f"pair_N{N}_B{B}"] = pair(B, N)
    rows["pair_d8_N64_B8"] = pair(8, 64, d=8)
    rows["pair_mask_N64_B8"] = pair(8, 64, mask=True)

    mms = {"f32": L.MM_F32, "bf16x3": L.MM_BF16X3, "bf16": L.MM_BF16}
    acts = {"relu": L.ACT_RELU, "elu": L.ACT_ELU, "lrelu": L.ACT_LRELU}
    for W in (8, 16, 32, 40, 48, 64):
        for mm_name, mm in mms.items():
            for act_name, act in acts.items():
                for nrows in (1, 100, 128 * 64 * 64):   # zinc500k_n64: B * N * N edge rows
                    desc = L.FfnDesc(rows=nrows, width=W, dtype=L.EGT_F32, activation=act, ln_eps=1e-3, matmul=mm, flags=0)
                    rows[f"ffn_W{W}_{mm_name}_{act_name}_rows{nrows}"] = lib.egt_ffn_workspace_bytes(C.byref(desc))
    return rows


def test_op_workspace_matches_golden(egt_lib):
    got = table(egt_lib)
    want = json.load(open(GOLDEN))
    assert set(got) == set(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"workspace bytes: got vs golden {bad}"


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from egt_amd import _lib
    rows = table(_lib.load())
    print("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(rows[k])}" for k in sorted(rows)) + "\n}")
