#!/usr/bin/env python3
"""The large-head block operator (egt_pair_block_fwd / egt_pair_block_bwd: the node side of mha_block on the library's fp32 MFMA
GEMMs) measured in one visit; every measurement is a FRESH child process (the route switch is read once per process) under its own
time limit, and the first child that fails ends the run.

    python tools/bench_pair_block.py --parent-tree PARENT [--rounds 3] [--out profiles/pair_block.jsonl]

  (a) one block forward + backward at [8, 512, 512] and [32, 512, 512] (De = 32, random_mask_prob 0.1, training mode), node side
      "library" against node side "torch"; median of 20 timed steps after warm-up.  The library child also records every node-side
      kernel per launch (the library's launch profiler) with the TF/s its shape implies (2 M N K over the kernel time).
  (b) bench.py --workload synthetic_n512_block and synthetic_n512_block_b32: the parent tree, this tree as it routes by default,
      and this tree with the library node side switched on (EGT_PAIR_NODE=1), alternating over --rounds.
  (c) the guard: the headline bench.py line of both trees, same rounds.
Verdicts are worded against the parent's own spread (max - min over its rounds), as tools/bench_scale_degree.py words them.
Output: one JSON line per measurement, then the comparison / verdict lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "EGT_PAIR_NODE"
LEAN = ["--no-cpu-baseline", "--no-prof", "--no-graph-leg"]      # the timed window alone: no CPU baseline, profiler leg or replay leg
DH, D3 = 512, 1536
# floating-point operations of each GEMM-shaped kernel per node row
FLOP_PER_ROW = {"k_pn_qkv": 2 * DH * D3, "k_pn_out": 2 * DH * DH, "k_pn_dvatt": 2 * DH * DH, "k_pn_dln": 2 * D3 * DH,
                "k_pn_wgrad": 2 * DH * (D3 + DH)}
KERNELS = ("k_pn_stats", "k_pn_qkv", "k_pn_out", "k_pn_dvatt", "k_pn_dln", "k_pn_lnbwd", "k_pn_wgrad", "k_pn_reduce", "k_pair_fwd", "k_pair_bwd",
           "k_attn_pack", "k_attn_mfma_bwd_q")


def _timed(step, steps, warmup):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def child_block(args, B, node):
    sys.path.insert(0, os.getcwd())      # the tree this child was started in
    import torch
    from egt_amd import EGTBlock, _lib
    from egt_amd.pair import block_pair
    lib = _lib.load()
    N, dev = 512, torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    h = torch.randn(B, N, DH, generator=g).to(dev).requires_grad_(); e = torch.randn(B, N, N, 32, generator=g).to(dev).requires_grad_()
    mask = torch.ones(B, N, dtype=torch.bool, device=dev)
    dh, de = torch.randn_like(h), torch.randn_like(e)
    torch.manual_seed(0)
    blk = EGTBlock(model_width=DH, edge_width=32, num_heads=8, random_mask_prob=0.1).to(dev).train()

    def fn():
        h.grad = e.grad = None
        for p in blk.parameters():
            p.grad = None
        h2, e2 = block_pair(blk, h, e, mask, node=node)
        torch.autograd.backward([h2, e2], [dh, de])
    rec = dict(case="block", B=B, N=N, node=node, steps=args.steps)
    rec["ms_per_step"], rec["steps_ms"] = _timed(fn, args.steps, args.warmup)
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    lib.egt_prof_enable(0)
    ks = {}
    for nm in KERNELS:
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(nm.encode(), C.byref(cnt), C.byref(ms))
        if cnt.value:
            us = ms.value / cnt.value * 1e3
            ks[nm] = dict(launches=cnt.value, us_per_launch=round(us, 2))
            if nm in FLOP_PER_ROW:
                ks[nm]["tflops"] = round(FLOP_PER_ROW[nm] * B * N / us * 1e-6, 1)
    rec["kernels"] = ks
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_block.jsonl"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--child", default=None, help="(internal) block:<B>:<library|torch>")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--skip", default="", help="comma list of a, b, c")
    args = ap.parse_args()
    if args.child:
        _, B, node = args.child.split(":")
        return child_block(args, int(B), node)
    me, recs, skip = os.path.abspath(__file__), [], set(args.skip.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = open(args.out, "w")

    def emit(o):               # kept as it comes: a child that fails later loses nothing measured before it
        recs.append(o)
        print(json.dumps({k: v for k, v in o.items() if k != "steps_ms"}), flush=True)
        sink.write(json.dumps(o) + "\n"); sink.flush()

    def run(cmd, tree, env_extra, tag):
        env = dict(os.environ, **env_extra)
        for k in ("EGT_AMD_LIB",) + (() if SWITCH in env_extra else (SWITCH,)):
            env.pop(k, None)
        r = subprocess.run([sys.executable] + cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:      # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {cmd[1:]} ({tag}) failed with exit status {r.returncode}; nothing more is run")
        out = []
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                out.append(dict(json.loads(line[7:]), **tag))
            elif line.startswith("{") and "ms_per_step" in line:      # bench.py's result line
                d = json.loads(line)
                out.append(dict(case="bench.py " + tag["workload"], ms_per_step=d["ms_per_step"], median_ms_per_step=d.get("median_ms_per_step"),
                                value=d.get("value"), metric=d.get("metric"), **tag))
        for o in out:
            emit(o)
        return out

    common = ["--steps", str(args.steps), "--warmup", str(args.warmup)]
    if "a" not in skip:
        for B in (8, 32):
            for node in ("library", "torch"):
                run([me, "--child", f"block:{B}:{node}"] + common, REPO, {}, dict(part="a"))
        for B in (8, 32):
            t = {r["node"]: r["ms_per_step"] for r in recs if r.get("part") == "a" and r["B"] == B}
            c = dict(compare="a", case="block", B=B, library_ms=t["library"], torch_ms=t["torch"], speedup=round(t["torch"] / t["library"], 3))
            emit(c)
    med = lambda v: sorted(v)[len(v) // 2]
    ok = True
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    arms = ([(parent, "parent", {})] if parent else []) + [(REPO, "this", {}), (REPO, "this+library", {SWITCH: "1"})]
    bench = lambda wl: ["bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "10"] + (["--workload", wl] if wl else [])
    for rnd in range(args.rounds):
        for tree, tag, env in arms:
            if "b" not in skip:
                for wl in ("synthetic_n512_block", "synthetic_n512_block_b32"):
                    run(bench(wl) + LEAN, tree, env, dict(part="b", tree=tag, round=rnd, workload=wl))
            if "c" not in skip and tag != "this+library":
                run(bench(None) + LEAN, tree, env, dict(part="c", tree=tag, round=rnd, workload="headline"))
    runs = [r for r in recs if r.get("part") in ("b", "c")]
    for wl in dict.fromkeys(r["workload"] for r in runs):
        sel = lambda t: [r["ms_per_step"] for r in runs if r["workload"] == wl and r["tree"] == t]
        par = sel("parent")
        if not par:
            continue
        spread = max(par) - min(par)
        for arm in ("this", "this+library"):
            new = sel(arm)
            if not new:
                continue
            good = med(new) <= med(par) + spread
            if arm == "this":          # what the tree does by default must hold; the switched-on arm decides the default route
                ok &= good
            v = dict(workload=wl, arm=arm, figure="ms_per_step", parent=par, this=new, parent_median=med(par), this_median=med(new),
                     parent_spread=spread, verdict="within the parent's spread" if good else "SLOWER than the parent's spread allows")
            emit(v)
    sink.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
