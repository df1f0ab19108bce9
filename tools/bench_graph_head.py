#!/usr/bin/env python3
"""Graph-level readout head (ZINC / CIFAR10 readout: node_norm_final, pooling, MLP, loss, metric sums): the fused kernels
against the composed torch head, and what the head is worth to a training step -- on the same GPU in the same run, every
measurement in a FRESH child process (EGT_NO_GRAPH_HEAD is read once per process).

(a) op scope: forward + backward of the head alone on h [B,nv+N,W], fused (egt_graph_head_fwd / _bwd) against composed
    (graph_head_composed), at [128,64,64] MAE, [128,37,48] MAE, [128,150,64] XENT (10 classes) and [128,1+64,64] MAE with one
    virtual node.
(b) model scope: one training step (forward + loss + backward into a flat gradient buffer) of the ZINC-500k (N = 64, widths
    64 / 64, 10 layers), ZINC-100k (N = 37, widths 48 / 48, 4 layers) and CIFAR10 (N = 150, widths 64 / 8, 4 layers, bf16 edges)
    models at B = 128, eager and replayed from a captured hipGraph: in this tree (model.graph_loss), in this tree under
    EGT_NO_GRAPH_HEAD=1, and -- with --parent-tree DIR, a built checkout of the parent commit -- in that tree (loss_fn(model(..)),
    the step of before).  --rounds R repeats the three of every case R times, alternating.
Every figure is the median of `--steps` individually timed iterations after `--warmup` untimed ones; a comparison takes the
median of the R per-round medians.  Against the parent the margin is the parent's own spread: the largest minus the smallest of
its per-round medians.

    python tools/bench_graph_head.py [--out profiles/graph_head.jsonl] [--steps 20] [--warmup 5] [--parent-tree DIR] [--rounds 3]

Output: one JSON line per measurement (with its tree and round), then one comparison line per row."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_SHAPES = {"op_mae_n64_w64": (128, 64, 64, "mae", 1, 0), "op_mae_n37_w48": (128, 37, 48, "mae", 1, 0),     # B, N, W, loss, C, nv
             "op_xent_n150_w64": (128, 150, 64, "xent", 10, 0), "op_mae_n64_w64_nv1": (128, 64, 64, "mae", 1, 1)}
MODELS = {"zinc_500k": ("zinc", 64, 64, 10, 64, 38, "f32"), "zinc_100k": ("zinc", 48, 48, 4, 37, 9, "f32"),
          "cifar10": ("cifar10", 64, 8, 4, 150, 85, "bf16")}       # kind, Dh, De, layers, N, fewest nodes, edge dtype


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
    sys.path.insert(0, args.tree)
    from egt_amd.graph_head import graph_head_loss, graph_head_composed
    from egt_amd.layers import KerasDense, KerasLayerNorm
    B, N, W, loss, Cn, nv = OP_SHAPES[args.child]
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
    mask = torch.cat([torch.ones(B, nv, dtype=torch.bool), torch.arange(N)[None, :] < n[:, None]], dim=1).to(dev)
    h = torch.randn(B, nv + N, W, generator=g).to(dev).requires_grad_()
    y = (torch.randn(B, Cn, generator=g) if loss == "mae" else torch.randint(0, Cn, (B,), generator=g)).to(dev)
    torch.manual_seed(0)
    ln, d0, d1, dt = (KerasLayerNorm(W).to(dev), KerasDense(max(nv, 1) * W, W // 2).to(dev), KerasDense(W // 2, W // 4).to(dev),
                      KerasDense(W // 4, Cn).to(dev))
    params = (ln.gamma, ln.beta, d0.kernel, d0.bias, d1.kernel, d1.bias, dt.kernel, dt.bias)
    for route, fn in (("fused", graph_head_loss), ("composed", graph_head_composed)):
        def step():
            h.grad = None
            for p in params:
                p.grad = None
            st, _ = fn(h, y, mask, params, loss, nv, "elu")
            st[0].backward()
        med, ts = _timed(step, args.warmup, args.steps)
        print("RESULT " + json.dumps(dict(scope="op", case=args.child, tree=args.tree_name, shape=[B, nv + N, W], loss=loss, C=Cn, nv=nv,
                                          route=route, steps=args.steps, ms=med, min_ms=min(ts), max_ms=max(ts))), flush=True)


def child_step(args):
    import torch
    sys.path.insert(0, args.tree)
    from egt_amd import Cifar10DCTransformer, ZincDCTransformer, mae_loss, sparse_xent_loss
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.graph import DeviceSeeds, GraphedStep
    kind, Dh, De, Ly, N, lo, edt = MODELS[args.child]
    B, dev = args.B, torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    n = torch.randint(lo, N + 1, (B,), generator=g); n[0] = N
    real = torch.arange(N)[None, :] < n[:, None]
    adj = (torch.rand(B, N, N, generator=g) > 0.94).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    if kind == "zinc":
        nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
        fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
        y, cls, loss_fn = torch.randn(B, 1, generator=g), ZincDCTransformer, mae_loss
    else:
        nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
        fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
        y, cls, loss_fn = torch.randint(0, 10, (B,), generator=g), Cifar10DCTransformer, sparse_xent_loss
    nf, fm, adj, y = (t.to(dev) for t in (nf, fm, adj, y))
    for graph in (False, True):
        torch.manual_seed(0)
        model = cls(model_width=Dh, edge_width=De, model_height=Ly, num_heads=8, upto_hop=16, random_mask_prob=0.1, seed=1,
                    edge_dtype=edt).to(dev).train()
        flat = FlatGradAllReduce(model.trainable_parameters(), direct=True)
        seen = {"head": "forward + loss_fn"}                # (a tree without graph_loss: the step of before)

        def fn():
            flat.zero(); flat.rebind()
            if hasattr(model, "graph_loss"):
                loss, stats, _, _ = model.graph_loss(nf, fm, adj, y)
                seen["head"] = type(stats.grad_fn).__name__
            else:
                loss = loss_fn(model(nf, fm, adj), y)
            loss.backward()
            return loss.detach()
        step = GraphedStep(fn, DeviceSeeds.attach(model, dev), warmup=1).replay if graph else fn
        med, ts = _timed(step, args.warmup, args.steps)
        print("RESULT " + json.dumps(dict(scope="step", model=args.child, tree=args.tree_name, layers=Ly, B=B, N=N, edge_dtype=edt,
                                          head=seen["head"], step_mode="hipgraph" if graph else "eager", steps=args.steps, ms=med,
                                          min_ms=min(ts), max_ms=max(ts))), flush=True)
        del model, flat, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "graph_head.jsonl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--only", default="op,step")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: every step is timed there too")
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of every step measurement (the trees alternating)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--tree-name", default="this")
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child in OP_SHAPES:
        return child_op(args)
    if args.child:
        return child_step(args)
    recs, rounds = [], {}       # rounds[("op", case, route) | ("step", model, mode)][tree name]: the per-round medians

    def run(child, tree, name, rnd, off=False):
        env = dict(os.environ)
        env.pop("EGT_NO_GRAPH_HEAD", None)
        if off:
            env["EGT_NO_GRAPH_HEAD"] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--B", str(args.B), "--tree", os.path.abspath(tree), "--tree-name", name]
        r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {child} (tree={name}) failed with exit status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                rec = dict(json.loads(line[7:]), round=rnd)
                recs.append(rec)
                key = ("op", rec["case"], rec["route"]) if rec["scope"] == "op" else ("step", rec["model"], rec["step_mode"])
                rounds.setdefault(key, {}).setdefault(name, []).append(rec["ms"])
                print(json.dumps(rec), flush=True)

    only = args.only.split(",")
    if "op" in only:
        for c in OP_SHAPES:
            run(c, REPO, "this", 0)
    if "step" in only:
        for m in args.models.split(","):
            for rnd in range(args.rounds):
                if args.parent_tree:
                    run(m, args.parent_tree, "parent", rnd)
                run(m, REPO, "this", rnd)
                run(m, REPO, "this_composed", rnd, off=True)
    med = lambda key, tree="this": statistics.median(rounds[key][tree])
    cmp_ = []
    for c in OP_SHAPES:
        if ("op", c, "fused") in rounds:
            f, b = med(("op", c, "fused")), med(("op", c, "composed"))
            cmp_.append(dict(compare=True, scope="op", case=c, fused_ms=f, composed_ms=b, ratio=round(b / f, 2),
                             gain_pct=round(100.0 * (b - f) / b, 2), fused_is_faster=f < b))
    for key, by_tree in rounds.items():
        if key[0] != "step":
            continue
        t, c = med(key), med(key, "this_composed")
        row = dict(compare=True, scope="step", model=key[1], step_mode=key[2], this_ms=t, composed_ms=c, this_round_ms=by_tree["this"],
                   composed_round_ms=by_tree["this_composed"], gain_vs_composed_pct=round(100.0 * (c - t) / c, 2))
        if "parent" in by_tree:      # this tree may be slower than the parent by no more than the parent's own spread over the rounds
            p, spread = med(key, "parent"), max(by_tree["parent"]) - min(by_tree["parent"])
            row.update(parent_ms=p, parent_round_ms=by_tree["parent"], parent_spread_ms=spread,
                       vs_parent_pct=round(100.0 * (t / p - 1.0), 2), no_slower=t - p <= spread)
        cmp_.append(row)
    for c in cmp_:
        print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
