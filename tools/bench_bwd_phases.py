#!/usr/bin/env python3
"""The pair kernels of the fused block, parent tree against this tree, on one GPU in one visit: the backward kernels (k_block_bwd_v4 /
v5 / v4r) or, with --kernel k_block_fwd, the forward ones (k_block_fwd / k_block_fwd_r4); with --kernel k_attn_mfma / k_pair the
d = 64, H = 8 family (k_attn_mfma_fwd + k_attn_mfma_bwd_kv / k_pair_fwd + k_pair_bwd: an entry names the kernels it records).

    python tools/bench_bwd_phases.py --parent-tree PARENT [--kernel k_block_bwd|k_block_fwd|k_attn_mfma|k_pair] [--rounds 3] [--out profiles/bwd_phases.jsonl]

PARENT is a built checkout of the parent commit.  Every measurement is a fresh child process under its own time limit, run in the
tree it measures; parent and this tree alternate over the rounds.  The first child that fails ends the run (nothing more is started on
the GPU).  Cases:
  bench.py --full --graph off workloads (the `kernels` figure of the kernel and the step time; the step mode is fixed to the eager
  stream because bench.py times the kernel by hipEvents on the stream there and by event nodes inside the captured graph otherwise, and
  the second way reads about 10 us more for the same code: a run that calibrates itself into the other mode is no comparison):
    zinc500k_n64                       k_block_bwd_v5<64>, full tiles;  k_block_fwd<64, true, false, true, false>
    zinc100k_n37                       k_block_bwd_v5<48>, ragged N, balanced ranges;  k_block_fwd<48, true, false, false, false>
    zinc500k_n64 --edge-dtype bf16     k_block_bwd_v4<64, false, true, false>;  k_block_fwd<64, true, false, true, true>
    cifar10_n150_fp32, EGT_NO_NARROW=1 k_block_bwd_v4r<8>                                                     (backward)
    cifar10_n150_fp32, EGT_NO_NARROW_FWD=1      k_block_fwd_r4<8, false, 8, false>                            (forward)
    pattern500k_n120_b128, EGT_NO_NARROW_FWD=1  k_block_fwd_r4<8, false, 4, false>                            (forward)
  single blocks: one block forward and backward through the C ABI on the buffers of tests/memcontract.py, the kernel timed by the
  library's own launch profiler (egt_prof_*); no bench.py workload reaches these instances:
    h [128, 64, 64], De = 64 with an attention mask   k_block_bwd_v4<64, true, false, false>;  k_block_fwd<64, true, true, false, false>
    h [32, 90, 64], De = 64 without one (forward)     k_block_fwd<64, false, false, false, false>: K / V do not fit in LDS
  k_attn_mfma / k_pair: synthetic_n512 (k_attn_mfma_fwd / _bwd_kv<64, 2>), synthetic_n512_block and synthetic_n512_block_nomask
  (k_pair_fwd / k_pair_bwd<64, 32, 2 | 1, true>); single cases on memcontract's mfma_case / pair_case at N = 69 -- five key tiles, the
  last one ragged: the smallest N at which every part of the pair kernels' trip structure runs (peeled first trip, one unrolled group of
  three steady forward trips / two backward ones, the remainder, the peeled last trip): k_attn_mfma_fwd / _bwd_kv<64, 1> and
  k_pair_fwd / k_pair_bwd<64, 32, 2 | 1, false> (V = 1: the case's descriptor with random_mask_prob = 0).
  Before the first round, every case's answer of egt_block_launch_form (in each tree, under the case's environment) goes into the file
  (the fused block's entries only).
Verdict per case and figure: this tree may be slower than the parent by no more than the parent's own spread (max - min over its
rounds)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z64, Z37, Z64B = (128, 64, 8, 64, False), (128, 37, 6, 48, False), (128, 64, 8, 64, True)      # (B, N, d, De, bf16) of the workload's block
MASK_ROW = ("b128_n64_de64_mask", 128, 64, 8, 64, False, "attn_mask", None, None)
# per kernel: bench.py cases (name, arguments, environment, block shape) and single-block cases (name, memcontract row)
CASES = {
    "k_block_bwd": dict(
        bench=[("zinc500k_n64", ["--workload", "zinc500k_n64"], {}, Z64),
               ("zinc100k_n37", ["--workload", "zinc100k_n37"], {}, Z37),
               ("zinc500k_n64_bf16", ["--workload", "zinc500k_n64", "--edge-dtype", "bf16"], {}, Z64B),
               ("cifar10_n150_fp32_no_narrow", ["--workload", "cifar10_n150_fp32"], {"EGT_NO_NARROW": "1"}, (128, 150, 8, 8, False))],
        single=[("mask_b128_n64_de64", MASK_ROW)]),
    "k_attn_mfma": dict(
        kernels=["k_attn_mfma_fwd", "k_attn_mfma_bwd_kv"], forms=False, out="attn_phases.jsonl",
        bench=[("synthetic_n512", ["--workload", "synthetic_n512"], {}, None)],
        single=[("mfma_b2_n69_d64", ("mfma", 2, 69, 64, False))]),
    "k_pair": dict(
        kernels=["k_pair_fwd", "k_pair_bwd"], forms=False, out="attn_phases.jsonl",
        bench=[("synthetic_n512_block", ["--workload", "synthetic_n512_block"], {}, None),
               ("synthetic_n512_block_nomask", ["--workload", "synthetic_n512_block_nomask"], {}, None)],
        single=[("pair_b2_n69_v2", ("pair", 2, 69, 61, False, True)), ("pair_b2_n69_v1", ("pair", 2, 69, 61, False, False))]),
    "k_block_fwd": dict(
        bench=[("zinc500k_n64", ["--workload", "zinc500k_n64"], {}, Z64),
               ("zinc100k_n37", ["--workload", "zinc100k_n37"], {}, Z37),
               ("zinc500k_n64_bf16", ["--workload", "zinc500k_n64", "--edge-dtype", "bf16"], {}, Z64B),
               ("cifar10_n150_fp32_no_narrow_fwd", ["--workload", "cifar10_n150_fp32"], {"EGT_NO_NARROW_FWD": "1"}, (128, 150, 8, 8, False)),
               ("pattern500k_n120_b128_no_narrow_fwd", ["--workload", "pattern500k_n120_b128"], {"EGT_NO_NARROW_FWD": "1"},
                (128, 120, 8, 8, False))],
        single=[("mask_b128_n64_de64", MASK_ROW), ("b32_n90_de64", ("b32_n90_de64", 32, 90, 8, 64, False, "", None, None))]),
}


def _tree_imports():
    sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tests")]      # the tree this child was started in
    import memcontract as M
    from egt_amd import _lib as L
    return M, L, L.load()


def child_forms(kernel, env):
    """the launch form of every case of `kernel` whose environment is `env` (this process's: the plan reads its switches once), in this
    process's tree; no GPU work"""
    M, L, lib = _tree_imports()
    cases = CASES[kernel]
    rows = [(name, e, ("", *shape, "", None, None)) for name, _, e, shape in cases["bench"]] + [(n, {}, r) for n, r in cases["single"]]
    for name, e, row in rows:
        if e == env:
            form = lib.egt_block_launch_form(C.byref(M.block_desc(row)))
            print(json.dumps(dict(case=name, env=env, form=form.decode() if form else None)))


def kernels_of(kernel):
    return CASES[kernel].get("kernels", [kernel])      # the kernels an entry records (their launch-profiler names)


def child_single(kernel, name, steps):
    M, L, lib = _tree_imports()
    import torch
    gpu = torch.device("cuda", 0)
    row = dict(CASES[kernel]["single"])[name]
    if row[0] == "mfma":
        case, form = M.mfma_case(lib, *row[1:]), None
    elif row[0] == "pair":
        case, form = M.pair_case(lib, *row[1:5]), None
        if not row[5]:
            case.claims["desc"].random_mask_prob = 0.0      # (the steps hold the descriptor by reference) V = 1: no in-kernel random mask
    else:
        case = M.block_case(lib, row)
        form = lib.egt_block_launch_form(C.byref(case.claims["desc"])).decode()
    M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check)          # warm-up
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    for _ in range(steps):
        M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
    lib.egt_prof_enable(0)
    rec = {"form": form, "launches": steps}
    for k in kernels_of(kernel):
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(k.encode(), C.byref(cnt), C.byref(ms))
        assert cnt.value == steps, (k, cnt.value)
        rec[k + "_us"] = ms.value / cnt.value * 1e3
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--kernel", choices=sorted(CASES), default="k_block_bwd")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mask-steps", type=int, default=8)
    ap.add_argument("--out", default=None, help="default: profiles/bwd_phases.jsonl, profiles/fwd_phases.jsonl for k_block_fwd, "
                                                "profiles/attn_phases.jsonl for k_attn_mfma and k_pair")
    ap.add_argument("--append", action="store_true", help="add to the file (a second entry of the same visit)")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child-single", default=None, help="(internal) the single-block case this child runs")
    ap.add_argument("--child-forms", default=None, help="(internal) print the launch form of every case of this environment (JSON)")
    args = ap.parse_args()
    if args.child_forms:
        return child_forms(args.kernel, json.loads(args.child_forms))
    if args.child_single:
        return child_single(args.kernel, args.child_single, args.mask_steps)
    kfigs, cases = [k + "_us" for k in kernels_of(args.kernel)], CASES[args.kernel]
    args.out = args.out or os.path.join(REPO, "profiles", cases.get("out", ("fwd" if args.kernel == "k_block_fwd" else "bwd") + "_phases.jsonl"))
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
            rec = {k + "_us": d["roofline"]["kernels"][k]["avg_us"] for k in kernels_of(args.kernel)}
            rec.update({"ms_per_step": d["ms_per_step"], "median_ms_per_step": d.get("median_ms_per_step"),
                        "step_mode": (d.get("config") or {}).get("step_mode")})
        else:
            rec = d
        rec = dict(case=name, tree=tag, round=rnd, env=env_extra, **rec)
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    me = os.path.abspath(__file__)
    envs = [json.loads(x) for x in dict.fromkeys(json.dumps(e, sort_keys=True) for _, _, e, _ in cases["bench"])]
    for tree, tag in trees if cases.get("forms", True) else []:
        for e in envs + ([] if {} in envs else [{}]):
            env = dict(os.environ, **e)
            env.pop("EGT_AMD_LIB", None)
            r = subprocess.run([sys.executable, me, "--kernel", args.kernel, "--child-forms", json.dumps(e)], cwd=tree, env=env,
                               capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:
                sys.stderr.write((r.stdout + r.stderr)[-4000:])
                raise SystemExit(f"launch forms ({tag}): child exit status {r.returncode}; nothing more is run")
            for l in r.stdout.splitlines():
                if l.startswith("{"):
                    recs.append(dict(tree=tag, **json.loads(l)))
                    print(json.dumps(recs[-1]), flush=True)
    for rnd in range(args.rounds):
        for tree, tag in trees:
            for name, extra, env, _ in cases["bench"]:
                run(name, tree, tag, rnd, ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--full",
                                          "--no-cpu-baseline", "--no-graph-leg", "--graph", "off"] + extra, env)
            for name, _ in cases["single"]:
                run(name, tree, tag, rnd, [me, "--kernel", args.kernel, "--child-single", name, "--mask-steps", str(args.mask_steps)], {})
    ok, runs = True, [r for r in recs if "round" in r]
    if args.parent_tree:
        for name in dict.fromkeys(r["case"] for r in runs):
            for fig in kfigs + ["ms_per_step"]:
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
    with open(args.out, "a" if args.append else "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
