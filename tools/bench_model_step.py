#!/usr/bin/env python3
"""Model scope of BASELINE config 3: one CIFAR10 training step -- edge embedding -> 4 layers (attention block + node / edge FFN)
-> final norm, pooling, MLP head -> cross-entropy, forward and backward -- at B = 128, N = 150 (node counts in [85, 150]),
in both edge dtypes, eager and replayed from a captured hipGraph (device-resident mask seeds, gradients in one flat buffer).
bench.py --scope model has no edge-dtype switch; this is its bf16 counterpart.

    python tools/bench_model_step.py [--steps K] [--warmup W] [--B 128] [--N 150]

Prints one JSON line per (edge dtype, step mode) and a last line with the bf16 / fp32 speedups."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egt_amd import Cifar10DCTransformer, sparse_xent_loss  # noqa: E402
from egt_amd.dp import FlatGradAllReduce  # noqa: E402
from egt_amd.graph import DeviceSeeds, GraphedStep  # noqa: E402


def batch(B, N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(85, N + 1, (B,), generator=g)
    real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
    adj = (torch.rand(B, N, N, generator=g) > 0.94).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
    y = torch.randint(0, 10, (B,), generator=g)
    return [t.to(dev) for t in (nf, fm, adj, y)]


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def run(edge_dtype, graph, args, dev):
    torch.manual_seed(0)
    model = Cifar10DCTransformer(model_width=64, edge_width=8, model_height=4, num_heads=8, upto_hop=16, random_mask_prob=0.1,
                                 seed=1, edge_dtype=edge_dtype).to(dev).train()
    params = model.trainable_parameters()
    nf, fm, adj, y = batch(args.B, args.N, dev)
    flat = FlatGradAllReduce(params, direct=True)

    def fn():
        flat.zero(); flat.rebind()
        loss = sparse_xent_loss(model(nf, fm, adj), y)
        loss.backward()
        return loss.detach()
    if graph:
        gs = GraphedStep(fn, DeviceSeeds.attach(model, dev), warmup=1)
        step = gs.replay
    else:
        step = fn
    ms = time_steps(step, args.steps, args.warmup)
    return dict(scope="model", workload="cifar10_n150 model step (embedding, 4 layers, head, loss; fwd+bwd)", edge_dtype=edge_dtype,
                step_mode="hipgraph" if graph else "eager", B=args.B, N=args.N, nodes=[85, args.N], steps=args.steps,
                ms_per_step=ms, graphs_per_s=args.B / ms * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--N", type=int, default=150)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    for graph in (False, True):
        for dt in ("f32", "bf16"):
            r = run(dt, graph, args, dev)
            res[(dt, graph)] = r
            print(json.dumps(r), flush=True)
    print(json.dumps({"speedup_bf16_over_f32": {m: res[("f32", g)]["ms_per_step"] / res[("bf16", g)]["ms_per_step"]
                                               for m, g in (("eager", False), ("hipgraph", True))}}))


if __name__ == "__main__":
    main()
