#!/usr/bin/env python3
"""EGT-Simple ('bias' edge channels, edge_width 8) model step, static-edge route against the per-layer route.

One training step -- edge embedding -> model_height layers (attention block + node FFN) -> final norm, head, loss; forward and
backward -- at the reference's EGT-Simple shapes: PATTERN (16 layers, N = 120 and 188) and CIFAR10 (4 layers, N = 150), B = 128,
fp32 and bf16 edge tensors, eager and replayed from a captured hipGraph.  Every shape runs twice in FRESH child processes (the
switch is read once per process): the static-edge route (EGT_BF_STATIC_EDGE kernels, chained edge gradient) and
EGT_NO_STATIC_EDGE=1 (the residual kernels on identity / zero parameters, one cut chain per layer).  A child reports the median
of its timing windows and the per-launch times of k_block_fwd / k_block_bwd (egt_prof_* events, an eager pass of their own).

    python tools/bench_egt_simple.py [--out profiles/egt_simple_model_step.jsonl] [--steps 10] [--windows 5] [--shapes a,b]

Output: one JSON line per (shape, route, edge dtype, step mode), then one comparison line per (shape, edge dtype, step mode)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"pattern_n120": ("pattern", 16, 120), "pattern_n188": ("pattern", 16, 188), "cifar10_n150": ("cifar10", 4, 150)}


def child(args):
    import torch
    sys.path.insert(0, REPO)
    from egt_amd import (Cifar10DCTransformer, PatternDCTransformer, sparse_xent_loss, weighted_sparse_xent_loss,
                         class_weights_from_sizes, _lib)
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.graph import DeviceSeeds, GraphedStep
    kind, Ly, N = SHAPES[args.child]
    B, dev = args.B, torch.device("cuda", 0)
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
    real = torch.arange(N)[None, :] < n[:, None]
    adj = (torch.rand(B, N, N, generator=g) > 0.94).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    if kind == "cifar10":
        nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
        fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
        y = torch.randint(0, 10, (B,), generator=g)
        inputs = [t.to(dev) for t in (nf, fm, adj)]
    else:
        nf = torch.randint(0, 3, (B, N), generator=g); nf[~real] = -1
        y = torch.randint(0, 2, (B, N), generator=g); y[~real] = 0
        inputs = [t.to(dev) for t in (nf, adj)]
        cw = class_weights_from_sizes([979220, 209900], device=dev)
    y = y.to(dev)
    route = "off" if os.environ.get("EGT_NO_STATIC_EDGE", "") not in ("", "0") else "static"
    for edt in ("f32", "bf16"):
        for graph in (False, True):
            torch.manual_seed(0)
            cls = Cifar10DCTransformer if kind == "cifar10" else PatternDCTransformer
            model = cls(model_width=64, edge_width=8, model_height=Ly, num_heads=8, upto_hop=16, random_mask_prob=0.1, seed=1,
                        edge_channel_type="bias", edge_dtype=edt).to(dev).train()
            flat = FlatGradAllReduce(model.trainable_parameters(), direct=True)

            def fn():
                flat.zero(); flat.rebind()
                if kind == "cifar10":
                    loss = sparse_xent_loss(model(*inputs), y)
                else:
                    logits, mask = model(*inputs, return_mask=True)
                    loss = weighted_sparse_xent_loss(logits, y, mask, cw)
                loss.backward()
                return loss.detach()
            step = GraphedStep(fn, DeviceSeeds.attach(model, dev), warmup=1).replay if graph else fn
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            wins = []
            for _ in range(args.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
                wins.append(e0.elapsed_time(e1) / args.steps)
            rec = dict(shape=args.child, route=route, edge_route=model.layers.last_edge_route, edge_dtype=edt,
                       step_mode="hipgraph" if graph else "eager", B=B, N=N, layers=Ly, steps=args.steps, windows=wins,
                       ms_per_step=statistics.median(wins), graphs_per_s=B / statistics.median(wins) * 1e3)
            if not graph:       # per-launch kernel times: an eager pass of its own with the launch profiler on
                lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                lib.egt_prof_enable(0)
                ks = {}
                for nm in ("k_block_fwd", "k_block_bwd"):
                    cnt, ms = C.c_int64(0), C.c_double(0.0)
                    lib.egt_prof_read(nm.encode(), C.byref(cnt), C.byref(ms))
                    if cnt.value:
                        ks[nm] = dict(launches=cnt.value, us_per_launch=round(ms.value / cnt.value * 1e3, 2))
                rec["kernels"] = ks
            print("RESULT " + json.dumps(rec), flush=True)
            del model, flat, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "egt_simple_model_step.jsonl"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.child:
        return child(args)
    recs = []
    for shape in args.shapes.split(","):
        for route in ("static", "off"):
            env = dict(os.environ)
            env.pop("EGT_NO_STATIC_EDGE", None)
            if route == "off":
                env["EGT_NO_STATIC_EDGE"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--windows", str(args.windows), "--B", str(args.B)]
            r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
                sys.stderr.write((r.stdout + r.stderr)[-3000:])
                raise SystemExit(f"child {shape} / {route} failed with exit status {r.returncode}")
            for line in r.stdout.splitlines():
                if line.startswith("RESULT "):
                    recs.append(json.loads(line[7:]))
                    print(line[7:], flush=True)
    cmp_ = []
    key = lambda r: (r["shape"], r["edge_dtype"], r["step_mode"])
    on = {key(r): r for r in recs if r["route"] == "static"}
    off = {key(r): r for r in recs if r["route"] == "off"}
    for k in on:
        if k in off:
            a, b = on[k]["ms_per_step"], off[k]["ms_per_step"]
            c = dict(compare=True, shape=k[0], edge_dtype=k[1], step_mode=k[2], static_ms=a, off_ms=b, gain_pct=round(100.0 * (b - a) / b, 2))
            cmp_.append(c)
            print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
