#!/usr/bin/env python3
"""config.resident_step against the three keys it composes -- steps/s of ``train_model`` epochs, every measurement in a FRESH
child process, one after another, on synthetic packed stores at the workloads' own shapes (tools/bench_device_data.py's
``make_store``: ZINC n 9..37, CIFAR10 n 85..150 with bf16 edge tensors, PATTERN n 44..188).

Arms, alternating within a round, --rounds rounds in one visit:
  parent    the parent commit's built tree (--parent-tree), use_hipgraph + fused_optimizer + device_dataset on
  keys      this tree, the same three keys on, resident_step off
  resident  this tree, resident_step on as well
  guard     this tree, all four keys off (eager step, host loader)
and the headline ``bench.py`` line of both trees once per round.  A child trains one epoch to warm up (kernels, record maps,
captured geometries), then times --epochs epochs (stream synchronised around each); its figure is batches / the fastest epoch,
and the median epoch is recorded beside it.  A timed epoch is a whole ``train_model`` epoch: it ends with the driver's
checkpoint write (model + optimizer state to disk), the same in every arm, which dilutes the difference between arms.
Verdicts (one ``compare`` line per case) are taken against the PARENT arm's own spread across rounds (largest minus smallest
steps/s): ``resident`` is a gain only outside that spread, "no slower" only inside it; ``keys`` must equal ``parent`` within it.

--cases defaults to zinc_b128,cifar10_b128.  pattern_b128 and pattern_b16 are built (name them to run them) but are not in the
default: the PATTERN-500k step at B = 128 ended in an illegal memory access in an earlier tree and its cause is not found
(DESIGN 4.6f), so it is not started again from here.  A failed child ends the run: nothing more is started on the GPU.

    python tools/bench_resident_step.py --parent-tree DIR [--rounds 3] [--out profiles/resident_step.jsonl] [--cases ...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from bench_device_data import WORK, make_store      # noqa: E402  (the stores and model shapes of the device-data benchmark)

# case -> (dataset of bench_device_data.WORK, B, batches per epoch, extra config)
CASES = {"zinc_b128": ("zinc", 128, 32, {}), "cifar10_b128": ("cifar10", 128, 8, dict(edge_dtype="bf16")),
         "pattern_b128": ("pattern", 128, 8, {}), "pattern_b16": ("pattern", 16, 32, {})}
THREE = ("use_hipgraph", "fused_optimizer", "device_dataset")
ARMS = {"parent": (THREE, False), "keys": (THREE, False), "resident": (THREE, True), "guard": ((), False)}


def child(args):
    sys.path.insert(0, args.tree)
    import torch
    import egt_amd.training as T
    name, B, _, extra = CASES[args.child]
    scheme, _, (Dh, De), Ly = WORK[name]
    cls = {"zinc": T.ZincSVDScheme, "cifar10": T.Cifar10SVDScheme, "pattern": T.PatternSVDScheme}[name]
    keys, resident = ARMS[args.arm]
    cfg = dict(scheme=scheme, model_name="bench", model_width=Dh, edge_width=De, model_height=Ly, upto_hop=16, num_svd_features=8,
               sel_svd_features=8, batch_size=B, random_mask_prob=0.1, dataset_path=args.store, num_epochs=1, save_best=False,
               save_path=tempfile.mkdtemp(dir=args.scratch), **extra, **{k: True for k in keys})
    if resident:
        cfg["resident_step"] = True                  # (the parent tree has no such key)
    torch.manual_seed(0)
    s = cls(cfg, device=torch.device("cuda", 0), print_fn=lambda *a: None)
    s.load_data(splits=("training",)); s.load_model(); s.load_state()
    s.train_model()                                  # the warm-up epoch
    times = []
    for e in range(2, 2 + args.epochs):
        s.config["num_epochs"] = e
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.train_model()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    n = len(s.trainset)
    graphs = len(getattr(s, "_graphs", {}) or {})
    print("RESULT " + json.dumps(dict(scope="epoch", case=args.child, arm=args.arm, B=B, batches=n, geometries=graphs,
                                      steps_per_s=round(n / min(times), 2), median_steps_per_s=round(n / statistics.median(times), 2),
                                      includes_checkpoint_write=True, epochs_s=[round(t, 4) for t in times],
                                      loss=s.history[-1]["loss"])), flush=True)
    torch.cuda.synchronize()                         # nothing in flight when the captured graphs go
    if getattr(s, "_graphs", None):
        s._graphs.clear()
    del s
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resident_step.jsonl"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="zinc_b128,cifar10_b128")
    ap.add_argument("--arms", default="parent,keys,resident,guard")
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per child, after the warm-up epoch")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--no-headline", action="store_true", help="leave the bench.py lines out")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "bench_resident_step"))
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--child", default=None)
    ap.add_argument("--arm", default="keys")
    ap.add_argument("--store", default=None)
    ap.add_argument("--tree", default=REPO)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):
        os.remove(args.out)
    recs = []
    arms = [a for a in args.arms.split(",") if a != "parent" or args.parent_tree]

    def keep(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    def run(cmd, cwd, what):
        r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            with open(args.out + ".failed_child.log", "w") as f:
                f.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {what} failed with exit status {r.returncode}")
        return r.stdout

    stores = {}
    for case in args.cases.split(","):
        name, B, batches, _ = CASES[case]
        stores[case] = os.path.join(args.scratch, f"{name}_{B}x{batches}.npz")
        if not os.path.exists(stores[case]):
            make_store(stores[case], name, batches * B)
    for rnd in range(args.rounds):
        for case in args.cases.split(","):
            for arm in arms:
                tree = os.path.abspath(args.parent_tree) if arm == "parent" else REPO
                out = run([sys.executable, os.path.abspath(__file__), "--child", case, "--arm", arm, "--store", stores[case], "--tree", tree,
                           "--epochs", str(args.epochs), "--scratch", args.scratch], tree, f"{case}/{arm}")
                for line in out.splitlines():
                    if line.startswith("RESULT "):
                        keep(dict(json.loads(line[7:]), round=rnd))
        if not args.no_headline:
            for tree_name, tree in (("parent", args.parent_tree), ("this", REPO)):
                if tree is None:
                    continue
                out = run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                          os.path.abspath(tree), f"bench.py/{tree_name}")
                line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
                full = json.loads(line)
                keep(dict(scope="headline", tree=tree_name, round=rnd,
                          bench={k: full[k] for k in ("metric", "value", "unit", "steps", "warmup", "median_ms_per_step", "value_at_median") if k in full}))
    med = statistics.median
    cmp_ = []
    for case in args.cases.split(","):
        by = {a: [r["steps_per_s"] for r in recs if r.get("scope") == "epoch" and r["case"] == case and r["arm"] == a] for a in ARMS}
        if not (by["keys"] and by["resident"]):
            continue
        ref = by["parent"] or by["keys"]
        spread = max(ref) - min(ref)
        k, r = med(by["keys"]), med(by["resident"])
        row = dict(compare=True, case=case, reference_arm="parent" if by["parent"] else "keys", reference_spread_steps_per_s=round(spread, 2),
                   keys_steps_per_s=k, resident_steps_per_s=r, keys_rounds=by["keys"], resident_rounds=by["resident"],
                   resident_vs_keys_pct=round(100.0 * (r / k - 1.0), 2),
                   verdict="gain outside the spread" if r - k > spread else ("slower, outside the spread" if k - r > spread else "no slower: inside the spread"))
        if by["parent"]:
            p = med(by["parent"])
            row.update(parent_steps_per_s=p, parent_rounds=by["parent"], keys_vs_parent_pct=round(100.0 * (k / p - 1.0), 2),
                       keys_equals_parent_within_spread=abs(k - p) <= spread)
        if by["guard"]:
            row.update(guard_steps_per_s=med(by["guard"]), guard_rounds=by["guard"])
        cmp_.append(row)
    head = {t: [r["bench"] for r in recs if r.get("scope") == "headline" and r["tree"] == t] for t in ("parent", "this")}
    if head["this"]:
        key = "value"
        if key in head["this"][0]:
            row = dict(compare=True, case="bench.py", metric=key, this=[b[key] for b in head["this"]], parent=[b[key] for b in head["parent"]])
            if head["parent"]:
                sp = max(row["parent"]) - min(row["parent"])
                row.update(parent_spread=sp, this_equals_parent_within_spread=abs(med(row["this"]) - med(row["parent"])) <= sp)
            cmp_.append(row)
    for c in cmp_:
        print(json.dumps(c), flush=True)
    with open(args.out, "a") as f:
        for c in cmp_:
            f.write(json.dumps(c) + "\n")


if __name__ == "__main__":
    main()
