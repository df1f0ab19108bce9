#!/usr/bin/env python3
"""Fused flat optimizer (egt_amd.optim.FlatOptimizer: egt_optim_prepare + egt_optim_step) against torch.optim, and what it is
worth to a training step -- on the same GPU in the same run, every measurement in a FRESH child process.

(a) op scope: one Adam update over the parameter lists of the ZINC-500k (widths 64 / 64, 10 layers) and PATTERN-500k (widths
    64 / 8, 16 layers) models, random gradients: FlatOptimizer, torch.optim.Adam as the training driver builds it, and
    torch.optim.Adam(fused=True) where the installed torch offers it.  Host time (the wall clock of step() alone, nothing
    synchronised inside) and device time (hipEvents around step()) separately, and the host cost of the stale-pointer check
    (FlatOptimizer.pointers_current) on its own.
(b) step scope: ``train_step`` of the ZINC-500k / PATTERN-500k schemes on one synthetic batch of B = 128, eager and with
    use_hipgraph, config.fused_optimizer on and off, and -- with --parent-tree DIR, a built checkout of the parent commit --
    in that tree (which has no such key).  Wall clock of the whole call (train_step ends on the loss read-back).  --rounds R
    repeats the arms of every case R times, alternating.  --step-models defaults to zinc_500k alone: the PATTERN-500k step
    (B = 128, N <= 120, 16 layers) of the PARENT commit's tree ended in an illegal memory access when this tool first ran it,
    before any arm of this tree had run; until that is understood the case is not run.
Every figure is the median of `--steps` individually timed iterations after `--warmup` untimed ones; a comparison takes the
median of the R per-round medians, and the verdict of a case is given against the off arm's own spread (largest minus
smallest of its per-round medians).

    python tools/bench_flat_optim.py [--out profiles/flat_optim.jsonl] [--steps 20] [--warmup 5] [--parent-tree DIR] [--rounds 3]

Output: one JSON line per measurement (with its tree and round), appended to --out as it arrives, then one comparison line per
row.  --summarize FILE recomputes the comparison lines from the measurement lines of FILE (a run that was cut short)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"zinc_500k": ("zinc", 64, 64, 10, (38, 64)), "pattern_500k": ("pattern", 64, 8, 16, (44, 120))}   # kind, Dh, De, layers, nodes


def _model(kind, Dh, De, Ly, dev):
    import torch
    from egt_amd import PatternDCTransformer, ZincDCTransformer
    torch.manual_seed(0)
    cls = ZincDCTransformer if kind == "zinc" else PatternDCTransformer
    return cls(model_width=Dh, edge_width=De, model_height=Ly, num_heads=8, upto_hop=16).to(dev)


def child_op(args):
    import torch
    sys.path.insert(0, args.tree)
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.optim import FlatOptimizer
    kind, Dh, De, Ly, _ = MODELS[args.child]
    dev = torch.device("cuda", 0)
    mk = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-7)
    arms = [("flat", None), ("torch_adam", {}), ("torch_adam_fused", dict(fused=True))]
    for route, kw in arms:
        params = _model(kind, Dh, De, Ly, dev).trainable_parameters()
        g = torch.Generator(device=dev).manual_seed(1)
        if kw is None:
            flat = FlatGradAllReduce(params, direct=True)
            flat.flat.copy_(torch.randn(flat.flat.shape, generator=g, device=dev) * 0.01)
            opt = FlatOptimizer(params, flat, algo="adam", lr=mk["lr"])
        else:
            for p in params:
                p.grad = torch.randn(p.shape, generator=g, device=dev) * 0.01
            try:
                opt = torch.optim.Adam(params, **mk, **kw)
                opt.step()
            except (RuntimeError, TypeError, ValueError) as e:      # this torch has no fused Adam for the device
                print("RESULT " + json.dumps(dict(scope="op", model=args.child, route=route, unavailable=str(e)[:200])), flush=True)
                continue
        for _ in range(args.warmup):
            opt.step()
        host, devt = [], []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(); opt.step(); b.record()
            host.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            devt.append(a.elapsed_time(b))
        rec = dict(scope="op", model=args.child, tree=args.tree_name, route=route, tensors=len(params),
                   elements=sum(p.numel() for p in params), steps=args.steps, host_ms=statistics.median(host),
                   device_ms=statistics.median(devt), host_min_ms=min(host), device_min_ms=min(devt))
        if kw is None:
            chk = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                ok = opt.pointers_current()
                chk.append((time.perf_counter() - t0) * 1e3)
            assert ok
            rec.update(work_items=opt._items, pointer_check_host_ms=statistics.median(chk))
        print("RESULT " + json.dumps(rec), flush=True)
        del opt, params


def child_step(args):
    import torch
    sys.path.insert(0, args.tree)
    import egt_amd.training as T
    kind, Dh, De, Ly, nodes = MODELS[args.child]
    B, dev = args.B, torch.device("cuda", 0)
    if kind == "zinc":
        cls, data = T.ZincSVDScheme, T.SyntheticZinc(B, B, nodes=nodes, seed=0)
    else:
        cls, data = T.PatternSVDScheme, T.SyntheticPattern(B, B, nodes=nodes, seed=0)
    batch = {k: v.to(dev) for k, v in next(iter(data)).items()}
    for graph in (False, True):
        torch.manual_seed(0)
        cfg = dict(scheme=f"{kind}.svd", model_name="bench", model_width=Dh, edge_width=De, model_height=Ly, upto_hop=16, use_svd=False,
                   batch_size=B, random_mask_prob=0.1, use_hipgraph=graph, save_path=os.path.join(args.scratch, "run"))
        if args.fused:
            cfg["fused_optimizer"] = True                    # (the parent tree has no such key)
        s = cls(cfg, device=dev, print_fn=lambda *a: None)
        s.load_model()
        for _ in range(args.warmup):
            s.train_step(batch)
        ts = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.train_step(batch)
            ts.append((time.perf_counter() - t0) * 1e3)
        print("RESULT " + json.dumps(dict(scope="step", model=args.child, tree=args.tree_name, layers=Ly, B=B, N=int(batch["graph_matrix"].shape[1]),
                                          optimizer=type(s.optimizer).__name__, step_mode="hipgraph" if graph else "eager",
                                          steps=args.steps, ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))), flush=True)
        del s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flat_optim.jsonl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--only", default="op,step")
    ap.add_argument("--models", default=",".join(MODELS), help="op scope")
    ap.add_argument("--step-models", default="zinc_500k", help="step scope")
    ap.add_argument("--summarize", default=None, help="no measurement: comparison lines from the measurement lines of this file")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: every step is timed there too")
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of every step measurement (the arms alternating)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-scope", default="step")
    ap.add_argument("--fused", type=int, default=0)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--tree-name", default="this")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "bench_flat_optim"))
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.child:
        return child_op(args) if args.child_scope == "op" else child_step(args)
    recs, rounds = [], {}       # rounds[("step", model, mode)][arm]: the per-round medians
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def take(rec):
        recs.append(rec)
        if rec["scope"] == "step":
            rounds.setdefault(("step", rec["model"], rec["step_mode"]), {}).setdefault(rec["tree"], []).append(rec["ms"])

    def run(child, scope, tree, name, rnd, fused=0):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--child-scope", scope, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--B", str(args.B), "--tree", os.path.abspath(tree), "--tree-name", name,
               "--fused", str(fused), "--scratch", args.scratch]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {child} (arm={name}) failed with exit status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                rec = dict(json.loads(line[7:]), round=rnd)
                take(rec)
                print(json.dumps(rec), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")

    only, models = args.only.split(","), args.models.split(",")
    if args.summarize:
        for line in open(args.summarize):
            if line.startswith("{") and '"compare"' not in line:
                take(json.loads(line))
        only = []
    elif os.path.exists(args.out):
        os.remove(args.out)
    if "op" in only:
        for m in models:
            run(m, "op", REPO, "this", 0)
    if "step" in only:
        for m in args.step_models.split(","):
            for rnd in range(args.rounds):
                if args.parent_tree:
                    run(m, "step", args.parent_tree, "parent", rnd)
                run(m, "step", REPO, "off", rnd)
                run(m, "step", REPO, "on", rnd, fused=1)
    cmp_ = []
    for m in models:
        ops = {r["route"]: r for r in recs if r["scope"] == "op" and r["model"] == m and "host_ms" in r}
        if "flat" in ops and "torch_adam" in ops:
            f, t = ops["flat"], ops["torch_adam"]
            row = dict(compare=True, scope="op", model=m, flat_host_ms=f["host_ms"], torch_host_ms=t["host_ms"], flat_device_ms=f["device_ms"],
                       torch_device_ms=t["device_ms"], pointer_check_host_ms=f["pointer_check_host_ms"],
                       host_ratio=round(t["host_ms"] / f["host_ms"], 2), device_ratio=round(t["device_ms"] / f["device_ms"], 2))
            if "torch_adam_fused" in ops:
                row.update(torch_fused_host_ms=ops["torch_adam_fused"]["host_ms"], torch_fused_device_ms=ops["torch_adam_fused"]["device_ms"])
            cmp_.append(row)
    med = lambda key, arm: statistics.median(rounds[key][arm])
    for key, by in rounds.items():
        if "on" not in by or "off" not in by:
            continue
        on, off = med(key, "on"), med(key, "off")
        spread = max(by["off"]) - min(by["off"])
        row = dict(compare=True, scope="step", model=key[1], step_mode=key[2], on_ms=on, off_ms=off, on_round_ms=by["on"], off_round_ms=by["off"],
                   off_spread_ms=spread, gain_pct=round(100.0 * (off - on) / off, 2),
                   verdict="faster" if off - on > spread else ("slower" if on - off > spread else "within the off arm's spread"))
        if "parent" in by:
            p = med(key, "parent")
            row.update(parent_ms=p, parent_round_ms=by["parent"], off_vs_parent_pct=round(100.0 * (off / p - 1.0), 2),
                       off_no_slower_than_parent=off - p <= max(by["parent"]) - min(by["parent"]))
        cmp_.append(row)
    for c in cmp_:
        print(json.dumps(c), flush=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
