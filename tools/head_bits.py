#!/usr/bin/env python3
"""A sha256 per output tensor of the fused edge head and node head, over the cases of tests/test_distance_head_gpu.py and
tests/test_node_head_gpu.py (their CASES, the bf16 and the full-tile case), for comparing two builds of the library bit by bit.
One process loads one library: run it once per build (each run under its own time limit, chained with &&) and diff the listings.

    python tools/head_bits.py [--lib path/to/libegt_amd.so] > listing.txt      (--lib: the EGT_AMD_LIB of this process)

Edge head: per_graph, d_e and the parameter gradients; node head: stats, d_h and the parameter gradients (two without LayerNorm)."""
import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        os.environ["EGT_AMD_LIB"] = os.path.abspath(args.lib)      # read when egt_amd._lib is imported
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import torch
    import test_distance_head_gpu as TD
    import test_node_head_gpu as TN
    from egt_amd.node_head import node_head_loss
    gpu = torch.device("cuda", 0)

    def emit(tag, out, first, grad_in, names):
        tensors = [(first, out[first]), (grad_in, out[grad_in])] + [("d " + n, g) for n, g in zip(names, out["grads"])]
        for name, t in tensors:
            raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
            print(f"{hashlib.sha256(raw).hexdigest()}  {tag} {name} {str(t.dtype)[6:]}{list(t.shape)}", flush=True)

    edge = [(c, {}) for c in TD.CASES] + [((8, 64, 3, "relu", True), dict(dtype=torch.bfloat16)), ((64, 64, 3, "elu", True), dict(N=16))]
    for case, kw in edge:
        got = TD._run_case(gpu, *case, **kw)[0]
        tag = "edge " + "-".join(map(str, case)) + "".join(f" {k}={str(v).replace('torch.', '')}" for k, v in kw.items())
        emit(tag, got, "per_graph", "d_e", TD.DR.HEAD_NAMES if case[4] else TD.DR.HEAD_NAMES[2:])
    for case in TN.CASES:
        x, params, _ = TN._reference(case)
        got, _ = TN._run(node_head_loss, x, params, case[3], gpu)
        emit("node " + "-".join(map(str, case)), got, "stats", "d_h", TN.NR.NAMES if case[4] else TN.NR.NAMES[2:])


if __name__ == "__main__":
    main()
