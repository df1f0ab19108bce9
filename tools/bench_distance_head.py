#!/usr/bin/env python3
"""Distance objective (egt_amd/head.py): the fused edge-head loss kernels against the same head composed from torch ops,
forward + backward, in one process, alternating, device-event timing after warm-up -- at the head shapes of the reference's
egt_spe_do configs (ZINC 500k: B=128 N=37 De=64; CIFAR10: B=128 N=150 De=8 in both edge dtypes, width 64, T=3) -- and the
model step of the two configs with the objective on and off.

    python tools/bench_distance_head.py [--steps K] [--warmup W] [--rounds R] [--out profiles/distance_head.jsonl]

One JSON line per measurement, printed and written to --out.  Algorithmic bytes: forward B N^2 (De sizeof(e) + 1) (e and the
uint8 targets), backward 2 B N^2 De sizeof(e) + B N^2 (e, d_e, targets); roofs 8 TB/s and 157.3 TFLOP/s (fp32 matrix)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egt_amd import ZincDCTransformer, Cifar10DCTransformer, mae_loss, sparse_xent_loss, distance_target  # noqa: E402
from egt_amd.head import DistanceHead, distance_head_composed  # noqa: E402

HBM_TBPS, MFMA_TF = 8.0, 157.3


def graphs(B, N, lo, p, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(lo, N + 1, (B,), generator=g)
    real = torch.arange(N)[None, :] < n[:, None]
    adj = (torch.rand(B, N, N, generator=g) < p).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    return adj, real, g


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench_head(B, N, De, width, T, edge_dtype, lo, p, args, dev):
    torch.manual_seed(0)
    dt = torch.bfloat16 if edge_dtype == "bf16" else torch.float32
    adj, _, _ = graphs(B, N, lo, p)
    target = distance_target(adj.to(dev), T)
    head = DistanceHead(De, width, T, edge_dtype=dt).to(dev)
    e = torch.randn(B, N, N, De, device=dev).to(dt).requires_grad_()
    s = torch.rand(B, device=dev) + 0.5
    params = head.params()

    def clear():
        e.grad = None
        for q in params:
            q.grad = None

    def fused(bwd=True):
        clear()
        out = head(e, target)
        if bwd:
            out.backward(s)

    def composed(bwd=True):
        clear()
        out = distance_head_composed(e, target, params, "elu")
        if bwd:
            out.backward(s)

    for _ in range(args.warmup):
        fused(); composed()
    torch.cuda.synchronize()
    ms = {"fused": [], "composed": [], "fused_fwd": [], "composed_fwd": []}
    for _ in range(args.rounds):                 # alternating: both see the same clocks and the same neighbours
        ms["fused"].append(timed(fused, args.steps))
        ms["composed"].append(timed(composed, args.steps))
        ms["fused_fwd"].append(timed(lambda: fused(False), args.steps))
        ms["composed_fwd"].append(timed(lambda: composed(False), args.steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    pairs, esz = B * N * N, e.element_size()
    m0, m1, C_ = round(.5 * width), round(.25 * width), T + 1
    bytes_fwd = pairs * (De * esz + 1)
    bytes_bwd = 2 * pairs * De * esz + pairs
    flop_fwd = 2 * pairs * (De * m0 + m0 * m1 + m1 * C_)
    flop_all = flop_fwd + 3 * flop_fwd           # the step: forward, then recompute + d inputs + d weights
    bwd_ms = med["fused"] - med["fused_fwd"]
    return dict(scope="distance_head", B=B, N=N, De=De, model_width=width, T=T, edge_dtype=edge_dtype, steps=args.steps,
                rounds=args.rounds, active_pair_fraction=float((target > 0).float().mean()),
                fused_ms=med["fused"], composed_ms=med["composed"], fused_fwd_ms=med["fused_fwd"], composed_fwd_ms=med["composed_fwd"],
                fused_ms_rounds=ms["fused"], composed_ms_rounds=ms["composed"],
                speedup=med["composed"] / med["fused"], speedup_fwd=med["composed_fwd"] / med["fused_fwd"],
                bytes_algorithmic_fwd=bytes_fwd, bytes_algorithmic_bwd=bytes_bwd, flops_fwd=flop_fwd, flops_step=flop_all,
                frac_hbm_roof_fwd=bytes_fwd / (med["fused_fwd"] * 1e-3) / (HBM_TBPS * 1e12),
                frac_hbm_roof_bwd=bytes_bwd / (max(bwd_ms, 1e-6) * 1e-3) / (HBM_TBPS * 1e12),
                frac_mfma_roof_step=flop_all / (med["fused"] * 1e-3) / (MFMA_TF * 1e12))


def bench_model(kind, edge_dtype, on, args, dev):
    torch.manual_seed(0)
    kw = dict(distance_loss=(0.05 if kind == "zinc" else 0.0005), distance_target=3) if on else {}
    if kind == "zinc":       # configs/main/zinc/500k/egt_spe_do.json (upto_hop at the scheme default 1)
        B, N = 128, 37
        model = ZincDCTransformer(model_width=64, edge_width=64, model_height=10, upto_hop=1, random_mask_prob=0.1, seed=1,
                                  edge_dtype=edge_dtype, **kw).to(dev).train()
        adj, real, g = graphs(B, N, 9, 0.08)
        nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
        fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
        y = torch.randn(B, 1, generator=g)
        loss_fn = mae_loss
    else:                    # configs/main/cifar10/100k/egt_spe_do.json
        B, N = 128, 150
        model = Cifar10DCTransformer(model_width=64, edge_width=8, model_height=4, upto_hop=1, random_mask_prob=0.1, seed=1,
                                     edge_dtype=edge_dtype, **kw).to(dev).train()
        adj, real, g = graphs(B, N, 85, 0.03)
        nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
        fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
        y = torch.randint(0, 10, (B,), generator=g)
        loss_fn = sparse_xent_loss
    nf, fm, adj, y = (t.to(dev) for t in (nf, fm, adj, y))
    params = model.trainable_parameters()

    def step():
        for q in params:
            q.grad = None
        if on:
            out, aux = model(nf, fm, adj, return_aux=True)
            loss = loss_fn(out, y) + kw["distance_loss"] * aux["distance_loss"].mean()
        else:
            loss = loss_fn(model(nf, fm, adj), y)
        loss.backward()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = sorted(timed(step, args.steps) for _ in range(args.rounds))
    return dict(scope="model_step", model=kind, B=B, N=N, edge_dtype=edge_dtype, distance_objective=on, ms_per_step=ms[len(ms) // 2],
                ms_rounds=ms, graphs_per_s=B / ms[len(ms) // 2] * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-models", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "distance_head.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    emit(bench_head(128, 37, 64, 64, 3, "f32", 9, 0.08, args, dev))
    emit(bench_head(128, 150, 8, 64, 3, "f32", 85, 0.03, args, dev))
    emit(bench_head(128, 150, 8, 64, 3, "bf16", 85, 0.03, args, dev))
    if not args.no_models:
        for kind, dts in (("zinc", ("f32",)), ("cifar10", ("f32", "bf16"))):
            for dt in dts:
                for on in (False, True):
                    emit(bench_model(kind, dt, on, args, dev))
    heads = [r for r in lines if r["scope"] == "distance_head"]
    emit(dict(scope="summary", bar="fused beats composed by more than 3 % at every head shape",
              speedups=[r["speedup"] for r in heads], met=all(r["speedup"] > 1.03 for r in heads)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
