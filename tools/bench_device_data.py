#!/usr/bin/env python3
"""Device-resident datasets (egt_amd.device_data, k_batch_assemble) against the host pipeline (egt_amd.data.GraphDataset) --
every measurement in a FRESH child process, on synthetic packed stores at the workloads' own shapes (ZINC N <= 37 with 8 SVD
features, CIFAR10 N <= 150, PATTERN N <= 188; B = 128).

(1) loader:  batches/s of ``GraphDataset.batches(device=...)`` alone (prefetch thread on, records cached: the second and
             third epoch; the first epoch, which pays the per-record maps, is reported separately) and of
             ``DeviceGraphDataset`` alone (pack + upload reported separately); ``step``: steps/s of ``train_step`` on one
             resident batch.  Together they say whether the host pipeline bounds an epoch.
(2) epoch:   wall clock of ``train_model`` over --epoch-batches batches (the faster of the second and third epoch of the
             process: kernels warm, records cached), ``device_dataset`` off and on, and -- with --parent-tree DIR, a built
             checkout of the parent commit -- "off" in that tree.  Eager steps; --graph-datasets adds the ``use_hipgraph`` arm.
(3) kernel:  ``k_batch_assemble`` per launch through egt_prof_* against ``fill_`` of the same output tensors in the same
             process (hipEvents around the fills of one batch), with the bytes written and read.
--rounds R repeats every arm R times, alternating; a comparison takes the median of the per-round figures and is judged
against the reference arm's own spread (largest minus smallest).  ``train_step`` children run for the ZINC and CIFAR10 schemes
only (--step-datasets): the PATTERN step at B = 128 is left out for the reason DESIGN 4.6f gives.

    python tools/bench_device_data.py [--out profiles/device_data.jsonl] [--rounds 3] [--parent-tree DIR] [--only loader,step,epoch,kernel]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# dataset -> (scheme, node range, model widths (Dh, De), layers)
WORK = {"zinc": ("zinc.svd", (9, 37), (64, 64), 10), "cifar10": ("cifar10.svd", (85, 150), (64, 64), 4),
        "pattern": ("pattern.svd", (44, 188), (64, 8), 16)}
SPEC = {"zinc": "zinc", "cifar10": "cifar10", "pattern": "sbm_pattern"}


def make_store(path, name, n_graphs, seed=0):
    """a synthetic packed store in the workload's shape (host only)"""
    sys.path.insert(0, REPO)
    from egt_amd import data as D
    rng = np.random.default_rng(seed)
    lo, hi = WORK[name][1]

    def record():
        n = int(rng.integers(lo, hi + 1))
        if name == "zinc":          # a chain with a few ring closures, both directions, bond types 0..2
            pairs = {(i, i + 1) for i in range(n - 1)} | {(i, i + 5) for i in range(0, n - 5, 7)}
        elif name == "cifar10":     # 8 nearest neighbours of random positions
            pos = rng.random((n, 2))
            d = ((pos[:, None] - pos[None]) ** 2).sum(-1) + np.eye(n) * 10
            nb = np.argsort(d, axis=1)[:, :8]
            pairs = {(i, int(j)) for i in range(n) for j in nb[i]}
        else:                       # two communities, about 25 neighbours per node
            adj = np.triu(rng.random((n, n)) < 25.0 / n, 1)
            pairs = {(int(i), int(j)) for i, j in zip(*np.nonzero(adj))}
        pairs = sorted(pairs)
        if name == "cifar10":
            edges = np.asarray(pairs, np.int32).reshape(-1, 2)
            rec = dict(edges=edges, node_features=rng.random((n, 5), dtype=np.float32),
                       edge_features=rng.random((len(edges), 1), dtype=np.float32), target=np.int32(rng.integers(0, 10)))
        else:
            edges = np.asarray(pairs + [(j, i) for i, j in pairs], np.int32).reshape(-1, 2)
            if name == "zinc":
                ef = rng.integers(0, 3, size=len(pairs)).astype(np.int32)
                nf = rng.integers(0, 28, size=n).astype(np.int32)
                rec = dict(edges=edges, node_features=nf, edge_features=np.concatenate([ef, ef]),
                           target=np.asarray([nf.sum() / 100.0], np.float32))
            else:
                rec = dict(edges=edges, node_features=rng.integers(0, 3, size=n).astype(np.int32),
                           target=rng.integers(0, 2, size=n).astype(np.int32))
        rec["num_nodes"] = np.int32(n)
        return rec
    spec = D.SPECS[SPEC[name]]
    D.write_packed_store(path, spec.db_name, dict(training=[record() for _ in range(n_graphs)], validation=[record() for _ in range(128)]),
                         {f.name: f.key for f in spec.fields}, meta=dict(num_graphs=n_graphs + 128))


def _dataset(args, **kw):
    from egt_amd.data import dataset_for_scheme
    return dataset_for_scheme(WORK[args.child][0], args.store, num_svd_features=8, use_svd=True, seed=1, splits=("training",), **kw)


def _result(args, **rec):
    print("RESULT " + json.dumps(dict(dataset=args.child, tree=args.tree_name, B=args.B, **rec)), flush=True)


def child_loader(args):
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    t0 = time.perf_counter()
    ds = _dataset(args)
    src = ds.to_device(dev) if args.mode == "device" else ds
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    epochs, n, shape = [], 0, None
    for _ in range(3):
        t0 = time.perf_counter()
        n = 0
        for b in src.get_batched_data(args.B, device=dev):
            n += 1
            shape = tuple(b["graph_matrix"].shape)
        torch.cuda.synchronize()
        epochs.append(time.perf_counter() - t0)
    _result(args, scope="loader", mode=args.mode, batches=n, last_shape=shape, setup_s=round(setup, 3), first_epoch_s=round(epochs[0], 4),
            batches_per_s=round(n / statistics.median(epochs[1:]), 1), steady_epoch_s=[round(e, 4) for e in epochs[1:]],
            resident_bytes=getattr(src, "nbytes", None))


def _scheme(args, graph, on, **extra):
    import torch
    import egt_amd.training as T
    scheme, _, (Dh, De), Ly = WORK[args.child]
    cls = {"zinc": T.ZincSVDScheme, "cifar10": T.Cifar10SVDScheme}[args.child]
    cfg = dict(scheme=scheme, model_name="bench", model_width=Dh, edge_width=De, model_height=Ly, upto_hop=16, num_svd_features=8,
               sel_svd_features=8, batch_size=args.B, random_mask_prob=0.1, use_hipgraph=graph, dataset_path=args.store,
               save_path=tempfile.mkdtemp(dir=args.scratch), **extra)          # (a fresh directory: no checkpoint to resume from)
    if on:
        cfg["device_dataset"] = True                 # (the parent tree has no such key)
    torch.manual_seed(0)
    return cls(cfg, device=torch.device("cuda", 0), print_fn=lambda *a: None)


def child_step(args):
    import torch
    dev = torch.device("cuda", 0)
    batch = {k: v.to(dev) for k, v in next(iter(_dataset(args, prefetch_batch=False).get_batched_data(args.B))).items()}
    for graph in (False, True):
        s = _scheme(args, graph, False)
        s.load_model()
        for _ in range(args.warmup):
            s.train_step(batch)
        ts = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.train_step(batch)
            ts.append(time.perf_counter() - t0)
        _result(args, scope="step", step_mode="hipgraph" if graph else "eager", N=int(batch["graph_matrix"].shape[1]),
                ms=round(statistics.median(ts) * 1e3, 4), steps_per_s=round(1.0 / statistics.median(ts), 1))
        del s


def child_epoch(args):
    import torch
    for graph in ((False, True) if args.child in args.graph_datasets.split(",") else (False,)):
        s = _scheme(args, graph, bool(args.on), num_epochs=1, save_best=False)
        s.load_data(splits=("training",)); s.load_model(); s.load_state()
        s.train_model()                              # first epoch: record maps, kernels, captured geometries
        times = []
        for e in (2, 3):
            s.config["num_epochs"] = e
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.train_model()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        _result(args, scope="epoch", step_mode="hipgraph" if graph else "eager", arm=args.tree_name, batches=len(s.trainset),
                epoch_s=round(min(times), 4), epochs_s=[round(t, 4) for t in times], loss=s.history[-1]["loss"])
        del s


def child_kernel(args):
    import torch
    from egt_amd import _lib as L
    dev = torch.device("cuda", 0)
    src = _dataset(args).to_device(dev)
    lib = L.load()
    ids = list(range(args.B))
    out = src.assemble("training", ids)
    for _ in range(5):
        src.assemble("training", ids)
    torch.cuda.synchronize()
    lib.egt_prof_filter(b"k_batch_assemble"); lib.egt_prof_enable(2)
    for _ in range(args.steps):
        src.assemble("training", ids)
    torch.cuda.synchronize()
    lib.egt_prof_enable(0)
    cnt, ms = C.c_int64(0), C.c_double(0.0)
    lib.egt_prof_read(b"k_batch_assemble", C.byref(cnt), C.byref(ms))
    fills = []
    for _ in range(args.steps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in out.values():
            t.fill_(0)
        b.record()
        torch.cuda.synchronize()
        fills.append(a.elapsed_time(b))
    one = []                                        # the largest tensor alone: a fill without the gaps between launches
    big = max(out.values(), key=lambda t: t.numel())
    for _ in range(args.steps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); big.fill_(0); b.record()
        torch.cuda.synchronize()
        one.append(a.elapsed_time(b))
    sp = src._splits["training"]
    written = sum(t.numel() * t.element_size() for t in out.values())
    n = sp.num_nodes_host[ids].astype(np.int64)
    e = np.diff(sp.store["edge_off"].cpu().numpy())[ids]
    words = e * (2 if "edge_feat" in sp.store else 1) + n * (2 + sp.kinds["node_width"] + 16 + 1)
    kernel_ms, fill_ms = ms.value / max(cnt.value, 1), statistics.median(fills[5:])
    _result(args, scope="kernel", N=int(out["graph_matrix"].shape[1]), launches=cnt.value, kernel_ms=round(kernel_ms, 5),
            fill_ms=round(fill_ms, 5), fill_tensors=len(out), largest_fill_ms=round(statistics.median(one[5:]), 5),
            largest_bytes=big.numel() * big.element_size(), bytes_written=written, bytes_read=int(words.sum() * 4),
            ratio=round(kernel_ms / fill_ms, 3), write_GBps=round(written / kernel_ms / 1e6, 1))


CHILDREN = dict(loader=child_loader, step=child_step, epoch=child_epoch, kernel=child_kernel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_data.jsonl"))
    ap.add_argument("--only", default="loader,step,epoch,kernel")
    ap.add_argument("--datasets", default="zinc,cifar10,pattern", help="loader and kernel scope")
    ap.add_argument("--step-datasets", default="zinc,cifar10", help="step and epoch scope (train_step runs)")
    ap.add_argument("--loader-batches", type=int, default=16)
    ap.add_argument("--epoch-batches", type=int, default=64)
    ap.add_argument("--graph-datasets", default="", help="epoch scope: datasets whose use_hipgraph arm is timed too.  None by default: "
                    "the first such child (ZINC, the parent commit's tree, host loader) ended in an illegal memory access (DESIGN 4.6g)")
    ap.add_argument("--append", action="store_true", help="add to the measurement lines already in --out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the epoch is timed there too")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "bench_device_data"))
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-scope", default="loader")
    ap.add_argument("--mode", default="host")
    ap.add_argument("--on", type=int, default=0)
    ap.add_argument("--store", default=None)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--tree-name", default="this")
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, args.tree)
        return CHILDREN[args.child_scope](args)
    os.makedirs(args.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    recs = []
    if os.path.exists(args.out):
        if args.append:             # keep the measurement lines of an earlier invocation (another scope, another --epoch-batches)
            recs = [json.loads(ln) for ln in open(args.out) if ln.startswith("{") and '"compare"' not in ln]
        else:
            os.remove(args.out)

    def store(name, batches):
        path = os.path.join(args.scratch, f"{name}_{batches}.npz")
        if not os.path.exists(path):
            make_store(path, name, batches * args.B)
        return path

    def run(name, scope, path, rnd, tree=REPO, tree_name="this", mode="host", on=0):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--child-scope", scope, "--store", path, "--mode", mode,
               "--on", str(on), "--tree", os.path.abspath(tree), "--tree-name", tree_name, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--B", str(args.B), "--scratch", args.scratch, "--graph-datasets", args.graph_datasets]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:       # a failed child ends the run: nothing more is started on the GPU
            with open(args.out + ".failed_child.log", "w") as f:          # the whole output: the first error is at its top
                f.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
            sys.stderr.write((r.stdout + r.stderr)[:3000])
            raise SystemExit(f"child {name}/{scope} ({tree_name}, {mode}) failed with exit status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                rec = dict(json.loads(line[7:]), round=rnd)
                recs.append(rec)
                print(json.dumps(rec), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")

    only = args.only.split(",")
    for rnd in range(args.rounds):
        for name in args.datasets.split(","):
            if "loader" in only:
                run(name, "loader", store(name, args.loader_batches), rnd, mode="host")
                run(name, "loader", store(name, args.loader_batches), rnd, mode="device")
            if "kernel" in only and rnd == 0:
                run(name, "kernel", store(name, args.loader_batches), rnd)
        for name in args.step_datasets.split(","):
            if "step" in only:
                run(name, "step", store(name, args.loader_batches), rnd)
            if "epoch" in only:
                path = store(name, args.epoch_batches)
                if args.parent_tree:
                    run(name, "epoch", path, rnd, tree=args.parent_tree, tree_name="parent")
                run(name, "epoch", path, rnd, tree_name="off")
                run(name, "epoch", path, rnd, tree_name="on", on=1)
    med = statistics.median
    cmp_ = []
    for name in WORK:
        lo = {m: [r["batches_per_s"] for r in recs if r["scope"] == "loader" and r["dataset"] == name and r["mode"] == m] for m in ("host", "device")}
        if lo["host"] and lo["device"]:
            row = dict(compare=True, scope="loader", dataset=name, host_batches_per_s=med(lo["host"]), device_batches_per_s=med(lo["device"]),
                       host_rounds=lo["host"], device_rounds=lo["device"])
            for mode in ("eager", "hipgraph"):
                st = [r["steps_per_s"] for r in recs if r["scope"] == "step" and r["dataset"] == name and r["step_mode"] == mode]
                if st:
                    row[f"{mode}_steps_per_s"] = med(st)
                    row[f"host_loader_hidden_behind_{mode}_step"] = med(lo["host"]) > med(st)
            cmp_.append(row)
        for mode in ("eager", "hipgraph"):
            by = {a: [r["epoch_s"] for r in recs if r["scope"] == "epoch" and r["dataset"] == name and r["step_mode"] == mode and r["arm"] == a]
                  for a in ("parent", "off", "on")}
            if not (by["off"] and by["on"]):
                continue
            off, on = med(by["off"]), med(by["on"])
            row = dict(compare=True, scope="epoch", dataset=name, step_mode=mode, batches=sorted({r["batches"] for r in recs if r["scope"] == "epoch" and r["dataset"] == name}), off_s=off, on_s=on, off_rounds=by["off"], on_rounds=by["on"],
                       gain_pct=round(100.0 * (off - on) / off, 2))
            ref = by["parent"] or by["off"]
            spread = max(ref) - min(ref)
            row.update(reference_arm="parent" if by["parent"] else "off", reference_spread_s=round(spread, 4),
                       on_no_slower_than_off=on - off <= spread)
            if by["parent"]:
                p = med(by["parent"])
                row.update(parent_s=p, parent_rounds=by["parent"], off_vs_parent_pct=round(100.0 * (off / p - 1.0), 2),
                           off_equals_parent_within_spread=abs(off - p) <= spread)
            cmp_.append(row)
    for c in cmp_:
        print(json.dumps(c), flush=True)
    with open(args.out, "w") as f:
        for r in recs + cmp_:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
