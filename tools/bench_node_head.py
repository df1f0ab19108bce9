#!/usr/bin/env python3
"""Node-classification head (PATTERN / CLUSTER readout + class-weighted loss + metric sums): the fused kernels against the
composed torch head, on the same GPU in the same run.

(a) op scope: forward + backward of the head alone on h [B,N,64], fused (egt_node_head_fwd / _bwd) against composed
    (node_head_composed), at [128,188,64] with C = 2 and C = 6 and [128,150,64] with C = 6.
(b) step scope: one training step (model.classification_loss + backward into a flat gradient buffer) of the PATTERN and CLUSTER
    100k (4-layer) and 500k (16-layer) models at B = 128, default route against EGT_NO_NODE_HEAD=1, each in a FRESH child process
    (the switch is read once per process), eager and replayed from a captured hipGraph.
Every figure is the median of `--steps` individually timed iterations after `--warmup` untimed ones.

    python tools/bench_node_head.py [--out profiles/node_head.jsonl] [--steps 20] [--warmup 5] [--only op|step]

Output: one JSON line per measurement, then one comparison line per row (fused_ms / composed_ms / gain_pct)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_SHAPES = [(128, 188, 64, 2), (128, 188, 64, 6), (128, 150, 64, 6)]
MODELS = {"pattern_100k": ("pattern", 4, 188), "pattern_500k": ("pattern", 16, 188),
          "cluster_100k": ("cluster", 4, 190), "cluster_500k": ("cluster", 16, 190)}


def _timed(step, warmup, steps):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record(); step(); b.record()
    torch.cuda.synchronize()
    ts = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ts), ts


def child_op(args):
    import torch
    sys.path.insert(0, REPO)
    from egt_amd.node_head import node_head_loss, node_head_composed
    from egt_amd.layers import KerasDense, KerasLayerNorm
    dev = torch.device("cuda", 0)
    for B, N, W, Cn in OP_SHAPES:
        g = torch.Generator().manual_seed(0)
        n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
        mask = (torch.arange(N)[None, :] < n[:, None]).to(dev)
        h = (torch.randn(B, N, W, generator=g)).to(dev).requires_grad_()
        y = torch.randint(0, Cn, (B, N), generator=g).to(dev)
        cw = torch.full((Cn,), 1.0 / Cn, device=dev)
        torch.manual_seed(0)
        ln, d0, d1, dt = KerasLayerNorm(W).to(dev), KerasDense(W, W // 2).to(dev), KerasDense(W // 2, W // 4).to(dev), KerasDense(W // 4, Cn).to(dev)
        params = (ln.gamma, ln.beta, d0.kernel, d0.bias, d1.kernel, d1.bias, dt.kernel, dt.bias)
        for route, fn in (("fused", node_head_loss), ("composed", node_head_composed)):
            def step():
                h.grad = None
                for p in params:
                    p.grad = None
                st = fn(h, y, mask, cw, params, "elu")
                st[0].backward()
            med, ts = _timed(step, args.warmup, args.steps)
            print("RESULT " + json.dumps(dict(scope="op", shape=[B, N, W], C=Cn, route=route, steps=args.steps, ms=med,
                                              min_ms=min(ts), max_ms=max(ts))), flush=True)


def child_step(args):
    import torch
    sys.path.insert(0, REPO)
    from egt_amd import ClusterDCTransformer, PatternDCTransformer, class_weights_from_sizes
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.graph import DeviceSeeds, GraphedStep
    from egt_amd.node_head import node_head_disabled
    kind, Ly, N = MODELS[args.child]
    B, dev = args.B, torch.device("cuda", 0)
    Cn, feats = (2, 3) if kind == "pattern" else (6, 7)
    g = torch.Generator().manual_seed(0)
    n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
    real = torch.arange(N)[None, :] < n[:, None]
    adj = (torch.rand(B, N, N, generator=g) > 0.94).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    nf = torch.randint(0, feats, (B, N), generator=g); nf[~real] = -1
    y = torch.randint(0, Cn, (B, N), generator=g); y[~real] = 0
    nf, adj, y = nf.to(dev), adj.to(dev), y.to(dev)
    cw = class_weights_from_sizes([979220, 209900] if kind == "pattern" else [19695, 19222, 19559, 19417, 19801, 20139], device=dev)
    for graph in (False, True):
        torch.manual_seed(0)
        cls = PatternDCTransformer if kind == "pattern" else ClusterDCTransformer
        model = cls(model_width=64, edge_width=8, model_height=Ly, num_heads=8, upto_hop=16, random_mask_prob=0.1, seed=1).to(dev).train()
        flat = FlatGradAllReduce(model.trainable_parameters(), direct=True)
        seen = {}

        def fn():
            flat.zero(); flat.rebind()
            loss, stats, _ = model.classification_loss(nf, adj, y, cw)
            seen["head"] = type(stats.grad_fn).__name__
            loss.backward()
            return loss.detach()
        step = GraphedStep(fn, DeviceSeeds.attach(model, dev), warmup=1).replay if graph else fn
        med, ts = _timed(step, args.warmup, args.steps)
        print("RESULT " + json.dumps(dict(scope="step", model=args.child, layers=Ly, B=B, N=N, C=Cn,
                                          route="composed" if node_head_disabled() else "default", head=seen.get("head"),
                                          step_mode="hipgraph" if graph else "eager", steps=args.steps, ms=med, min_ms=min(ts),
                                          max_ms=max(ts))), flush=True)
        del model, flat, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "node_head.jsonl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--only", default="op,step")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child == "op":
        return child_op(args)
    if args.child:
        return child_step(args)
    recs = []

    def run(child, off):
        env = dict(os.environ)
        env.pop("EGT_NO_NODE_HEAD", None)
        if off:
            env["EGT_NO_NODE_HEAD"] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--B", str(args.B)]
        r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {child} (EGT_NO_NODE_HEAD={int(off)}) failed with exit status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                recs.append(json.loads(line[7:]))
                print(line[7:], flush=True)

    if "op" in args.only.split(","):
        run("op", False)
    if "step" in args.only.split(","):
        for m in args.models.split(","):
            for off in (False, True):
                run(m, off)
    cmp_ = []
    ops = {(tuple(r["shape"]), r["C"], r["route"]): r for r in recs if r["scope"] == "op"}
    for (shape, Cn, route), r in ops.items():
        if route == "fused" and (shape, Cn, "composed") in ops:
            b = ops[(shape, Cn, "composed")]["ms"]
            cmp_.append(dict(compare=True, scope="op", shape=list(shape), C=Cn, fused_ms=r["ms"], composed_ms=b,
                             gain_pct=round(100.0 * (b - r["ms"]) / b, 2), accept=r["ms"] <= b))
    st = {(r["model"], r["step_mode"], r["route"]): r for r in recs if r["scope"] == "step"}
    for (m, mode, route), r in st.items():
        if route == "default" and (m, mode, "composed") in st:
            b = st[(m, mode, "composed")]["ms"]
            cmp_.append(dict(compare=True, scope="step", model=m, step_mode=mode, default_ms=r["ms"], composed_ms=b, head=r["head"],
                             gain_pct=round(100.0 * (b - r["ms"]) / b, 2), accept=r["ms"] <= 1.03 * b))
    for c in cmp_:
        print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
