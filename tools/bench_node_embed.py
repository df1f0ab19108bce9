#!/usr/bin/env python3
"""Node-input embedding (lookup / Dense, SVD / eigenvector encoding, virtual rows -> h and mask): the fused kernels against the
composed torch ops -- on the same GPU in the same run, every case in a FRESH child process.

(a) op scope: forward + backward of the segment alone, fused (egt_node_embed_fwd / _bwd) against composed
    (node_embed_composed), at [128,64] -> 64 with SVD 8 of 16 (ZINC), [128,150,5] -> 64 with SVD (CIFAR10) and [128,188] -> 64
    with eigenvectors 2 of 20 (the PATTERN shape; op scope only).
(b) --count ROUTE with --child CASE: exactly --count-steps forward + backward passes of one route and nothing else, for a
    kernel trace around the process; the trace of 2 passes minus the trace of 1 is the launch list of one warm pass.
Every figure is the median of `--steps` individually timed iterations after `--warmup` untimed ones.
Step scope (a model's training step in this tree, under EGT_NO_NODE_EMBED=1 and in the parent commit's tree) is NOT part of this
tool: see DESIGN 4.6h.

    python tools/bench_node_embed.py [--out profiles/node_embed.jsonl] [--steps 20] [--warmup 5]

Output: one JSON line per measurement, then one comparison line per case."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# B, N, F (0: integer features), table rows, pe kind, sel, T, transform, nv
OP_SHAPES = {"op_zinc_n64_svd": (128, 64, 0, 29, "svd", 8, 16, True, 0), "op_cifar10_n150_svd": (128, 150, 5, 0, "svd", 8, 16, True, 0),
             "op_pattern_n188_eig": (128, 188, 0, 4, "eig", 2, 20, False, 0)}


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
    from egt_amd.node_embed import node_embed, node_embed_composed
    B, N, F, R, kind, sel, T, transform, nv = OP_SHAPES[args.child]
    Dh, dev = 64, torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
    real = torch.arange(N)[None, :] < n[:, None]
    if F:
        feat = torch.rand(B, N, F, generator=g); feat[~real] = -1.0
        emb, bias = torch.randn(F, Dh, generator=g) * 0.3, torch.zeros(Dh)
    else:
        feat = torch.randint(0, R - 1, (B, N), generator=g, dtype=torch.int32); feat[~real] = -1
        emb, bias = torch.empty(R, Dh).uniform_(-0.05, 0.05, generator=g), None
    pe = torch.randn(B, N, T, 2, generator=g) if kind == "svd" else torch.randn(B, N, T, generator=g)
    pe[~real] = 0.0
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_()
    emb, bias = leaf(emb), leaf(bias)
    dense = (leaf(torch.randn((2 if kind == "svd" else 1) * sel, Dh, generator=g) * 0.3), leaf(torch.zeros(Dh))) if transform else None
    vn = leaf(torch.empty(nv, Dh).uniform_(-0.05, 0.05, generator=g)) if nv else None
    feat, pe = feat.to(dev), pe.to(dev)
    d_h = torch.randn(B, nv + N, Dh, generator=g).to(dev)
    width = sel if transform else (Dh // 2 if kind == "svd" else Dh)
    params = [p for p in (emb, bias, *(dense or ()), vn) if p is not None]
    for route, fn in (("fused", node_embed), ("composed", node_embed_composed)):
        if args.count not in (None, route):
            continue

        def step():
            for p in params:
                p.grad = None
            sg = torch.where(torch.rand(B, 1, width, 1, device=dev) < 0.5, -1.0, 1.0)        # the model's draw, in both routes
            h, _ = fn(feat, emb, bias, pe, kind, sel, dense, sg if kind == "svd" else sg[..., 0], vn, -1.0)
            h.backward(d_h)
        if args.count:
            for _ in range(args.count_steps):
                step()
            torch.cuda.synchronize()
            print("COUNT-OK", args.child, route, args.count_steps, flush=True)
            continue
        med, ts = _timed(step, args.warmup, args.steps)
        print("RESULT " + json.dumps(dict(scope="op", case=args.child, tree=args.tree_name, shape=[B, nv + N, Dh], features=F or "int",
                                          pe=kind, sel=sel, T=T, transform=transform, nv=nv, route=route, steps=args.steps, ms=med,
                                          min_ms=min(ts), max_ms=max(ts))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "node_embed.jsonl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default=None, choices=list(OP_SHAPES))
    ap.add_argument("--count", default=None, choices=["fused", "composed"], help="with --child: only run --count-steps passes of this route")
    ap.add_argument("--count-steps", type=int, default=1)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--tree-name", default="this")
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child:
        return child_op(args)
    recs, by_case = [], {}
    for child in OP_SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        env = dict(os.environ)
        env.pop("EGT_NO_NODE_EMBED", None)
        r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"child {child} failed with exit status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                rec = json.loads(line[7:])
                recs.append(rec)
                by_case.setdefault(rec["case"], {})[rec["route"]] = rec["ms"]
                print(json.dumps(rec), flush=True)
    cmp_ = []
    for c, r in by_case.items():
        f, b = r["fused"], r["composed"]
        cmp_.append(dict(compare=True, scope="op", case=c, fused_ms=f, composed_ms=b, ratio=round(b / f, 2),
                         gain_pct=round(100.0 * (b - f) / b, 2), fused_is_faster=f < b))
    for c in cmp_:
        print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
