#!/usr/bin/env python3
"""The backward pair kernels of the fused block (k_block_bwd_v4 / v5 / v4r), parent tree against this tree, on one GPU in one visit.

    python tools/bench_bwd_phases.py --parent-tree PARENT [--rounds 3] [--out profiles/bwd_phases.jsonl]

PARENT is a built checkout of the parent commit.  Every measurement is a fresh child process under its own time limit, run in the
tree it measures; parent and this tree alternate over the rounds.  The first child that fails ends the run (nothing more is started on
the GPU).  Cases:
  bench.py --full --graph off workloads (the `kernels` figure of k_block_bwd and the step time; the step mode is fixed to the eager
  stream because bench.py times the kernel by hipEvents on the stream there and by event nodes inside the captured graph otherwise, and
  the second way reads about 10 us more for the same code: a run that calibrates itself into the other mode is no comparison):
    zinc500k_n64                       k_block_bwd_v5<64>, full tiles
    zinc100k_n37                       k_block_bwd_v5<48>, ragged N, balanced ranges
    zinc500k_n64 --edge-dtype bf16     k_block_bwd_v4<64, false, true, false>
    cifar10_n150_fp32, EGT_NO_NARROW=1 k_block_bwd_v4r<8>
  mask: one block forward and backward at h [128, 64, 64], De = 64 with an attention mask (k_block_bwd_v4<64, true, false, false>: no
    bench.py workload reaches the mask-tensor instances), through the C ABI on the buffers of tests/memcontract.py, k_block_bwd timed by
    the library's own launch profiler (egt_prof_*).
Verdict per case and figure: this tree may be slower than the parent by no more than the parent's own spread (max - min over its
rounds)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = [("zinc500k_n64", ["--workload", "zinc500k_n64"], {}),
         ("zinc100k_n37", ["--workload", "zinc100k_n37"], {}),
         ("zinc500k_n64_bf16", ["--workload", "zinc500k_n64", "--edge-dtype", "bf16"], {}),
         ("cifar10_n150_fp32_no_narrow", ["--workload", "cifar10_n150_fp32"], {"EGT_NO_NARROW": "1"})]
MASK_ROW = ("b128_n64_de64_mask", 128, 64, 8, 64, False, "attn_mask", None, None)


def child_mask(steps):
    sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tests")]      # the tree this child was started in
    import torch
    import memcontract as M
    from egt_amd import _lib as L
    lib = L.load()
    gpu = torch.device("cuda", 0)
    case = M.block_case(lib, MASK_ROW)
    form = lib.egt_block_launch_form(C.byref(case.claims["desc"])).decode()
    M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check)          # warm-up
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    for _ in range(steps):
        M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    lib.egt_prof_enable(0)
    cnt, ms = C.c_int64(0), C.c_double(0.0)
    lib.egt_prof_read(b"k_block_bwd", C.byref(cnt), C.byref(ms))
    assert cnt.value == steps, cnt.value
    print(json.dumps(dict(form=form, launches=cnt.value, k_block_bwd_us=ms.value / cnt.value * 1e3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mask-steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bwd_phases.jsonl"))
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child-mask", action="store_true")
    args = ap.parse_args()
    if args.child_mask:
        return child_mask(args.mask_steps)
    trees = ([(os.path.abspath(args.parent_tree), "parent")] if args.parent_tree else []) + [(REPO, "this")]
    recs = []

    def run(name, tree, tag, rnd, cmd, env_extra):
        env = dict(os.environ, **env_extra)
        env.pop("EGT_AMD_LIB", None)            # each tree loads its own library
        r = subprocess.run([sys.executable] + cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            sys.stderr.write((r.stdout + r.stderr)[-4000:])
            raise SystemExit(f"{name} ({tag}, round {rnd}): child exit status {r.returncode}; nothing more is run")
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        if "roofline" in d:
            rec = dict(k_block_bwd_us=d["roofline"]["kernels"]["k_block_bwd"]["avg_us"], ms_per_step=d["ms_per_step"],
                       median_ms_per_step=d.get("median_ms_per_step"), step_mode=(d.get("config") or {}).get("step_mode"))
        else:
            rec = d
        rec = dict(case=name, tree=tag, round=rnd, env=env_extra, **rec)
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    for rnd in range(args.rounds):
        for tree, tag in trees:
            for name, extra, env in BENCH:
                run(name, tree, tag, rnd, ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--full",
                                          "--no-cpu-baseline", "--no-graph-leg", "--graph", "off"] + extra, env)
            run("mask_b128_n64_de64", tree, tag, rnd, [os.path.abspath(__file__), "--child-mask", "--mask-steps", str(args.mask_steps)], {})
    ok, runs = True, list(recs)
    if args.parent_tree:
        for name in dict.fromkeys(r["case"] for r in runs):
            for fig in ("k_block_bwd_us", "ms_per_step"):
                par = [r[fig] for r in runs if r["case"] == name and r["tree"] == "parent" and fig in r]
                new = [r[fig] for r in runs if r["case"] == name and r["tree"] == "this" and fig in r]
                if not par:
                    continue
                spread = max(par) - min(par)
                med = lambda v: sorted(v)[len(v) // 2]
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
