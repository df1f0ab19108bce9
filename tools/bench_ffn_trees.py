#!/usr/bin/env python3
"""The channel FFN kernels (k_ffn_prep / k_ffn_fwd / k_ffn_bwd), parent tree against this tree, on one GPU in one visit.

    python tools/bench_ffn_trees.py --parent-tree PARENT [--rounds 3] [--out profiles/ffn_refactor.jsonl]

PARENT is a built checkout of the parent commit.  Every measurement is a fresh child process under its own time limit; parent and
this tree alternate over the rounds.  The first child that fails ends the run (nothing more is started on the GPU).  Cases:
  tools/bench_ffn.py of the tree it measures (its `kernels_us` of the three kernels and `ms_per_step`), arguments / product mode /
  storage:
    edge 128 64 64   f32     fp32
    edge 128 64 64   bf16x3  fp32
    edge 128 64 64   f32     bf16
    edge 128 37 48   f32     fp32
    node 128 64 64   f32     fp32      one tile per wave: the partial-reduction tail dominates
    edge 64 150 16   bf16x3  fp32
  headline: this tree's bench.py --gpus 1 --with-ffn --no-cpu-baseline with EGT_AMD_LIB at each tree's library (ms_per_step).
Verdict per case and figure: this tree may be slower than the parent by no more than the parent's own spread (max - min over its
rounds)."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join("egt_amd", "lib", "libegt_amd.so")
CASES = [("edge_128_64_64_f32", ["edge", "128", "64", "64"], {}),
         ("edge_128_64_64_bf16x3", ["edge", "128", "64", "64"], {"EGT_FFN_MATMUL": "bf16x3"}),
         ("edge_128_64_64_f32_bf16_storage", ["edge", "128", "64", "64"], {"EGT_FFN_DTYPE": "bf16"}),
         ("edge_128_37_48_f32", ["edge", "128", "37", "48"], {}),
         ("node_128_64_64_f32", ["node", "128", "64", "64"], {}),
         ("edge_64_150_16_bf16x3", ["edge", "64", "150", "16"], {"EGT_FFN_MATMUL": "bf16x3"})]
KERNELS = ("k_ffn_prep", "k_ffn_fwd", "k_ffn_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ffn_refactor.jsonl"))
    ap.add_argument("--child-timeout", type=int, default=180)
    args = ap.parse_args()
    trees = ([(os.path.abspath(args.parent_tree), "parent")] if args.parent_tree else []) + [(REPO, "this")]
    recs = []

    def run(name, tag, rnd, cmd, cwd, env_extra, lib=None):
        env = dict(os.environ, **env_extra)
        env.pop("EGT_AMD_LIB", None)            # bench_ffn.py: each tree loads its own library
        if lib:
            env["EGT_AMD_LIB"] = lib
        r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            sys.stderr.write((r.stdout + r.stderr)[-4000:])
            raise SystemExit(f"{name} ({tag}, round {rnd}): child exit status {r.returncode}; nothing more is run")
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        rec = dict(case=name, tree=tag, round=rnd, env=env_extra, ms_per_step=d["ms_per_step"])
        rec.update({k + "_us": d["kernels_us"][k] for k in KERNELS if k in d.get("kernels_us", {})})
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    for rnd in range(args.rounds):
        for tree, tag in trees:
            for name, argv, env in CASES:
                run(name, tag, rnd, [os.path.join("tools", "bench_ffn.py")] + argv, tree, env)
            run("bench_with_ffn", tag, rnd, ["bench.py", "--gpus", "1", "--with-ffn", "--steps", str(args.steps), "--warmup", str(args.warmup),
                                             "--no-cpu-baseline"], REPO, {}, lib=os.path.join(tree, LIB))
    ok, runs = True, list(recs)
    if args.parent_tree:
        med = lambda v: sorted(v)[len(v) // 2]
        for name in dict.fromkeys(r["case"] for r in runs):
            for fig in [k + "_us" for k in KERNELS] + ["ms_per_step"]:
                par = [r[fig] for r in runs if r["case"] == name and r["tree"] == "parent" and fig in r]
                new = [r[fig] for r in runs if r["case"] == name and r["tree"] == "this" and fig in r]
                if not par:
                    continue
                spread = max(par) - min(par)
                good = med(new) <= med(par) + spread
                ok &= good
                v = dict(case=name, figure=fig, verdict="within the parent's spread" if good else "SLOWER than the parent's spread allows",
                         parent=par, this=new, parent_median=med(par), this_median=med(new), parent_spread=spread)
                recs.append(v)
                print(json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
