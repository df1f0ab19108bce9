#!/usr/bin/env python3
"""Virtual nodes: the bordered edge embedding in one kernel against the same tensor composed from the existing op, and what
one virtual node costs a model step -- on the same GPU in the same run, every measurement in a FRESH child process.

(a) op scope: forward + backward of the embedding with nv = 1, fused (egt_edge_embed_vn_fwd / _bwd: one write of the
    [B,N',N',De] tensor, its gradient read once) against composed (edge_embed + two torch.cat passes, autograd's slice / pad
    backward), at [128,64,64,64] fp32 and [128,150,150,8] bf16 (upto_hop 16, a table of 5 rows), and at [128,150,150,8] bf16 with
    one real-valued feature plane and a table of one row: the CIFAR10 embedding (backward instance <17, 1, bf16>); and at
    [16,200,200,8] bf16, where the adjacency does not fit in LDS and the hop planes come from one k_hop_step launch per hop.
(b) step scope: one training step (forward + loss + backward into a flat gradient buffer, eager) of the ZINC-500k model
    (B = 128, N = 64, widths 64 / 64, 10 layers) and the CIFAR10 model (B = 128, N = 150, widths 64 / 8, 4 layers) at nv = 0
    and nv = 1.
--parent-tree DIR (a built checkout of the parent commit): every measurement is taken in that tree too, so that both values come
from one visit of one GPU; --rounds R repeats the parent / this pair of every measurement R times, alternating.
Every figure is the median of `--steps` individually timed iterations after `--warmup` untimed ones; a comparison takes the median
of the R per-round medians.  Against the parent the margin is the parent's own spread: the largest minus the smallest of its
per-round medians.

    python tools/bench_virtual_nodes.py [--out profiles/virtual_nodes.jsonl] [--steps 20] [--warmup 5] [--parent-tree DIR] [--rounds 3]

Output: one JSON line per measurement (with its tree and round), then one comparison line per row."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_SHAPES = {"op_f32_n64_de64": (128, 64, 64, "f32", 0), "op_bf16_n150_de8": (128, 150, 8, "bf16", 0),   # B, N, De, edge dtype, F
             "op_bf16_n150_de8_v1": (128, 150, 8, "bf16", 1), "op_bf16_n200_de8": (16, 200, 8, "bf16", 0)}
MODELS = {"zinc_500k": ("zinc", 64, 64, 10, 64, (38, 64)), "cifar10": ("cifar10", 64, 8, 4, 150, (85, 150))}
NV = 1


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


def _graphs(B, N, lo, g):
    import torch
    n = torch.randint(lo, N + 1, (B,), generator=g); n[0] = N
    real = torch.arange(N)[None, :] < n[:, None]
    adj = (torch.rand(B, N, N, generator=g) > 0.94).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    return real, adj


def child_op(args):
    import torch
    sys.path.insert(0, args.tree)
    from egt_amd import edge_embed
    B, N, De, edt, F = OP_SHAPES[args.child]
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    _, adj = _graphs(B, N, int(0.6 * N), g)
    fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
    shapes = [(5, De), (16, De), (De,), (NV, De)]
    if F:                                                 # real-valued features: no table index, F planes behind the hop planes
        fm, shapes = torch.full((B, N, N), -1), [(1, De)] + shapes[1:] + [(F, De), (De,)]
        ff = torch.rand(B, N, N, F, generator=g); ff[adj == 0] = -1.0
    fm, adj = fm.to(dev), adj.to(dev)
    prm = [torch.randn(s, generator=g).to(dev).requires_grad_() for s in shapes]
    table, W, b, vn = prm[:4]
    kw = dict(float_features=ff.to(dev), float_kernel=prm[4], float_bias=prm[5]) if F else {}
    dt = torch.bfloat16 if edt == "bf16" else torch.float32
    de = torch.randn(B, NV + N, NV + N, De, generator=g).to(dev).to(dt)

    def fused():
        return edge_embed(fm, adj, table, W, b, edge_dtype=edt, virtual_edge_table=vn, **kw)

    def composed():                                       # virtual_nodes.py:86-99 with torch ops around the existing op
        e = edge_embed(fm, adj, table, W, b, edge_dtype=edt, **kw)
        v = vn.to(dt)
        rows = v[None, :, None, :].expand(B, NV, N, De)
        cols = v[None, None, :, :].expand(B, N, NV, De)
        box = (0.5 * (vn[:, None, :] + vn[None, :, :])).to(dt)[None].expand(B, NV, NV, De)
        return torch.cat([torch.cat([box, cols], dim=1), torch.cat([rows, e], dim=1)], dim=2)
    out = {}
    for route, fn in (("fused", fused), ("composed", composed)):
        def step():
            for p in prm:
                p.grad = None
            fn().backward(de)
        med, ts = _timed(step, args.warmup, args.steps)
        out[route] = fn().detach().float()
        print("RESULT " + json.dumps(dict(scope="op", case=args.child, tree=args.tree_name, shape=[B, N, N, De], nv=NV, edge_dtype=edt,
                                          float_features=F, route=route, steps=args.steps, ms=med, min_ms=min(ts), max_ms=max(ts))), flush=True)
    assert torch.equal(out["fused"], out["composed"]), "the two routes must time the same result"


def child_step(args):
    import torch
    sys.path.insert(0, args.tree)
    from egt_amd import Cifar10DCTransformer, ZincDCTransformer, mae_loss, sparse_xent_loss
    from egt_amd.dp import FlatGradAllReduce
    kind, Dh, De, Ly, N, (lo, _) = MODELS[args.child]
    B, dev, nv = args.B, torch.device("cuda", 0), args.nv
    g = torch.Generator().manual_seed(0)
    real, adj = _graphs(B, N, lo, g)
    if kind == "zinc":
        nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
        fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
        y, cls, loss_fn = torch.randn(B, 1, generator=g), ZincDCTransformer, mae_loss
    else:
        nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
        fm = torch.rand(B, N, N, 1, generator=g); fm[adj == 0] = -1.0
        y, cls, loss_fn = torch.randint(0, 10, (B,), generator=g), Cifar10DCTransformer, sparse_xent_loss
    nf, fm, adj, y = (t.to(dev) for t in (nf, fm, adj, y))
    torch.manual_seed(0)
    model = cls(model_width=Dh, edge_width=De, model_height=Ly, num_heads=8, upto_hop=16, random_mask_prob=0.1, seed=1,
                num_virtual_nodes=nv).to(dev).train()
    flat = FlatGradAllReduce(model.trainable_parameters(), direct=True)

    def step():
        flat.zero(); flat.rebind()
        loss_fn(model(nf, fm, adj), y).backward()
    med, ts = _timed(step, args.warmup, args.steps)
    print("RESULT " + json.dumps(dict(scope="step", model=args.child, tree=args.tree_name, nv=nv, B=B, N=N, layers=Ly,
                                      paths=sorted({b.last_path for b in model.layers.blocks}), steps=args.steps, ms=med,
                                      min_ms=min(ts), max_ms=max(ts))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "virtual_nodes.jsonl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--only", default="op,step")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: every measurement is taken there too")
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of every measurement (parent / this alternating)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--tree-name", default="this")
    ap.add_argument("--nv", type=int, default=0)
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child in OP_SHAPES:
        return child_op(args)
    if args.child:
        return child_step(args)
    recs, rounds = [], {}       # rounds[("op", case, route) | ("step", model, nv)][tree name]: the per-round medians

    def run(child, nv, tree, name, rnd):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--B", str(args.B), "--nv", str(nv), "--tree", os.path.abspath(tree), "--tree-name", name]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {child} (nv={nv}, tree={name}) failed with exit status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                rec = dict(json.loads(line[7:]), round=rnd)
                recs.append(rec)
                key = ("op", rec["case"], rec["route"]) if rec["scope"] == "op" else ("step", rec["model"], rec["nv"])
                rounds.setdefault(key, {}).setdefault(name, []).append(rec["ms"])
                print(json.dumps(rec), flush=True)

    only = args.only.split(",")
    trees = ([(args.parent_tree, "parent")] if args.parent_tree else []) + [(REPO, "this")]
    for child, nv in [(c, 0) for c in OP_SHAPES if "op" in only] + [(m, nv) for m in MODELS for nv in (0, NV) if "step" in only]:
        for rnd in range(args.rounds):
            for tree, name in trees:
                run(child, nv, tree, name, rnd)
    med = lambda key, tree="this": statistics.median(rounds[key][tree])
    cmp_ = []
    for c in OP_SHAPES:
        if ("op", c, "fused") in rounds:
            f, b = med(("op", c, "fused")), med(("op", c, "composed"))
            cmp_.append(dict(compare=True, scope="op", case=c, fused_ms=f, composed_ms=b, gain_pct=round(100.0 * (b - f) / b, 2),
                             fused_is_faster=f < b))
    for m in MODELS:
        if ("step", m, 0) in rounds:
            n0, n1 = med(("step", m, 0)), med(("step", m, NV))
            cmp_.append(dict(compare=True, scope="step", model=m, nv0_ms=n0, nv1_ms=n1, nv1_cost_pct=round(100.0 * (n1 / n0 - 1.0), 2)))
    if args.parent_tree:        # this tree may be slower than the parent by no more than the parent's own spread over the rounds
        for key, by_tree in rounds.items():
            t, p, spread = med(key), med(key, "parent"), max(by_tree["parent"]) - min(by_tree["parent"])
            cmp_.append(dict(compare=True, against="parent", scope=key[0], case=key[1], **{"route" if key[0] == "op" else "nv": key[2]},
                             this_ms=t, parent_ms=p, parent_round_ms=by_tree["parent"], this_round_ms=by_tree["this"],
                             parent_spread_ms=spread, vs_parent_pct=round(100.0 * (t / p - 1.0), 2), no_slower=t - p <= spread))
    for c in cmp_:
        print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
