#!/usr/bin/env python3
"""Attention dropout (attn_dropout) on the fused route, measured in one visit; every measurement is a FRESH child process (the
switches are read once per process) under its own time limit, and the first child that fails ends the run.

    python tools/bench_attn_dropout.py [--parent-tree PARENT] [--rounds 3] [--out profiles/attn_dropout.jsonl]

  (a) one block forward + backward in training mode with attn_dropout = 0.1 and random_mask_prob = 0.1, B = 128, at [128, 64, 64]
      De = 64, [128, 37, 48] De = 48 and [128, 150, 64] De = 8 in fp32 and bf16: the opt-in fused route (fused_attn_dropout=True)
      against the composed route (fp32 only); median of 20 timed steps.  The fused child also records both pair kernels per launch
      (the library's launch profiler) with the flag and WITHOUT it (the same block with attn_dropout = 0: at De = 8 that twin runs
      the De = 8 VALU kernels, which the flagged descriptor leaves): the cost of the two extra hashes per lane and pair.
  (b) the ZINC-500K model step (10 layers, width 64, N = 64, B = 128, random_mask_prob 0.1, attn_dropout 0.1), both routes eager, and
      replayed from a hipGraph (the composed route cannot be captured -- its seed is a host argument -- and says so).
  (c) the guard: the same step with attn_dropout = 0 and the headline bench.py line, this tree against --parent-tree (a built checkout
      of the parent commit), alternating over --rounds; the verdict per case against the parent's own spread (max - min over its
      rounds), as tools/bench_scale_degree.py words it.
Output: one JSON line per measurement, then the comparison / verdict lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = {"n64_de64": (128, 64, 64, 64, "f32"), "n37_de48": (128, 37, 48, 48, "f32"), "n150_de8": (128, 150, 64, 8, "f32"),
          "n150_de8_bf16": (128, 150, 64, 8, "bf16")}      # B, N, Dh, De, edge dtype
RATE, PROB = 0.1, 0.1


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


def _pair_kernels(lib, fn, n=5):
    import torch
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    lib.egt_prof_enable(0)
    ks = {}
    for nm in ("k_block_fwd", "k_block_bwd"):
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(nm.encode(), C.byref(cnt), C.byref(ms))
        if cnt.value:
            ks[nm] = dict(launches=cnt.value, us_per_launch=round(ms.value / cnt.value * 1e3, 2))
    return ks


def child_block(args, shape, fused):
    sys.path.insert(0, os.getcwd())      # the tree this child was started in
    import torch
    from egt_amd import EGTBlock, _lib
    lib = _lib.load()
    B, N, Dh, De, edge = BLOCKS[shape]
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    h = torch.randn(B, N, Dh, generator=g).to(dev).requires_grad_()
    e = torch.randn(B, N, N, De, generator=g).to(dev).to(torch.bfloat16 if edge == "bf16" else torch.float32).requires_grad_()
    n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
    mask = (torch.arange(N)[None, :] < n[:, None]).to(dev)
    dh, de = torch.randn_like(h), torch.randn_like(e)
    rec = dict(case="block", shape=shape, B=B, N=N, Dh=Dh, De=De, edge=edge, attn_dropout=RATE, random_mask_prob=PROB, steps=args.steps)
    for sd in (True, False):            # sd: with the rate (the measured arm) | the same block with attn_dropout = 0 (pair kernels only)
        torch.manual_seed(0)
        blk = EGTBlock(model_width=Dh, edge_width=De, num_heads=8, attn_dropout=RATE if sd else 0.0, random_mask_prob=PROB,
                       fused_attn_dropout=fused).to(dev).train()

        def fn():
            h.grad = e.grad = None
            h2, e2 = blk(h, e, mask)
            torch.autograd.backward([h2, e2], [dh, de])
        fn()      # (the route is decided by the first call)
        if sd:
            rec["ms_per_step"], rec["steps_ms"] = _timed(fn, args.steps, args.warmup)
            rec["route"] = blk.last_path
        if fused and (blk.last_path == "fused" or not sd):
            rec["pair_kernels_flagged" if sd else "pair_kernels_unflagged"] = _pair_kernels(lib, fn)
        if not fused:
            break
    print("RESULT " + json.dumps(rec), flush=True)


def child_model(args, sd, fused=True):
    sys.path.insert(0, os.getcwd())
    import torch
    from egt_amd import ZincDCTransformer, mae_loss
    from egt_amd.dp import FlatGradAllReduce
    from egt_amd.graph import DeviceSeeds, GraphedStep
    B, N, dev = 128, 64, torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    n = torch.randint(9, 38, (B,), generator=g)
    real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
    adj = (torch.rand(B, N, N, generator=g) > 0.9).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
    y = torch.randn(B, 1, generator=g).to(dev)
    inputs = [t.to(dev) for t in (nf, fm, adj)]
    for graph in (False, True):
        torch.manual_seed(0)
        kw = dict(attn_dropout=RATE, **(dict(fused_attn_dropout=True) if fused else {})) if sd else {}      # (off: the parent's keywords only)
        model = ZincDCTransformer(model_width=64, edge_width=64, model_height=10, num_heads=8, upto_hop=16, random_mask_prob=0.1, seed=1,
                                  **kw).to(dev).train()
        flat = FlatGradAllReduce(model.trainable_parameters(), direct=True)

        def fn():
            flat.zero(); flat.rebind()
            loss = mae_loss(model(*inputs), y)
            loss.backward()
            return loss.detach()
        try:
            step = GraphedStep(fn, DeviceSeeds.attach(model, dev), warmup=1).replay if graph else fn
            ms, ts = _timed(step, args.steps, args.warmup)
        except RuntimeError as ex:      # the composed operator's mask seed is a host argument: no captured step on that route
            if not (graph and "DeviceSeeds" in str(ex)):
                raise
            print("RESULT " + json.dumps(dict(case="zinc500k_model_step", attn_dropout=RATE if sd else 0.0, step_mode="hipgraph", ms_per_step=None,
                                              unavailable="the composed route has no device-resident mask seeds: the step cannot be captured")), flush=True)
            continue
        paths = sorted({blk.last_path for blk in model.layers.blocks})
        print("RESULT " + json.dumps(dict(case="zinc500k_model_step", attn_dropout=RATE if sd else 0.0, routes=paths, step_mode="hipgraph" if graph else "eager",
                                          B=B, N=N, layers=10, steps=args.steps, ms_per_step=ms, steps_ms=ts, graphs_per_s=B / ms * 1e3)), flush=True)
        del model, flat, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_dropout.jsonl"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--child", default=None, help="(internal) block:<shape>:<fused|composed> | model:on:<fused|composed> | model:off")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--skip", default="", help="comma list of a, b, c")
    args = ap.parse_args()
    if args.child:
        kind, what, *arm = args.child.split(":")
        fused = not arm or arm[0] == "fused"
        return child_block(args, what, fused) if kind == "block" else child_model(args, what == "on", fused)
    me, recs, skip = os.path.abspath(__file__), [], set(args.skip.split(","))

    def run(cmd, tree, env_extra, tag):
        env = dict(os.environ, **env_extra)
        env.pop("EGT_AMD_LIB", None)
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
                out.append(dict(case="bench.py headline", ms_per_step=d["ms_per_step"], median_ms_per_step=d.get("median_ms_per_step"),
                                value=d.get("value"), metric=d.get("metric"), **tag))
        for o in out:
            recs.append(o)
            print(json.dumps({k: v for k, v in o.items() if k != "steps_ms"}), flush=True)
        return out

    common = ["--steps", str(args.steps), "--warmup", str(args.warmup)]
    for route in ("fused", "composed"):
        if "a" not in skip:
            for shape in BLOCKS:
                if route == "fused" or BLOCKS[shape][4] == "f32":      # (the composed route is fp32 only)
                    run([me, "--child", f"block:{shape}:{route}"] + common, REPO, {}, dict(part="a", want_route=route))
        if "b" not in skip:
            run([me, "--child", f"model:on:{route}"] + common, REPO, {}, dict(part="b", want_route=route))
    med = lambda v: sorted(v)[len(v) // 2]
    for part, key in (("a", lambda r: (r["shape"],)), ("b", lambda r: (r["step_mode"],))):
        on = {key(r): r for r in recs if r.get("part") == part and r["want_route"] == "fused"}
        off = {key(r): r for r in recs if r.get("part") == part and r["want_route"] == "composed"}
        for k in on:
            if k in off and off[k]["ms_per_step"] is not None:
                a, b = on[k]["ms_per_step"], off[k]["ms_per_step"]
                c = dict(compare=part, case=on[k]["case"], key=list(k), fused_ms=a, composed_ms=b, speedup=round(b / a, 3))
                recs.append(c); print(json.dumps(c), flush=True)
    for r in [r for r in recs if r.get("part") == "a" and r.get("pair_kernels_flagged") and r.get("pair_kernels_unflagged")]:
        fl, un = r["pair_kernels_flagged"], r["pair_kernels_unflagged"]
        c = dict(compare="flag cost", shape=r["shape"], edge=r["edge"],
                 **{f"{k}_flagged_over_unflagged": round(fl[k]["us_per_launch"] / un[k]["us_per_launch"], 3) for k in fl if k in un})
        recs.append(c); print(json.dumps(c), flush=True)
    ok = True
    if "c" not in skip:
        trees = ([(os.path.abspath(args.parent_tree), "parent")] if args.parent_tree else []) + [(REPO, "this")]
        for rnd in range(args.rounds):
            for tree, tag in trees:
                run([me, "--child", "model:off"] + common, tree, {}, dict(part="c", tree=tag, round=rnd))
                run(["bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "10"], tree, {}, dict(part="c", tree=tag, round=rnd))
        runs = [r for r in recs if r.get("part") == "c"]
        for name in dict.fromkeys((r["case"], r.get("step_mode")) for r in runs):
            sel = lambda t: [r["ms_per_step"] for r in runs if (r["case"], r.get("step_mode")) == name and r["tree"] == t]
            par, new = sel("parent"), sel("this")
            if not par:
                continue
            spread = max(par) - min(par)
            good = med(new) <= med(par) + spread
            ok &= good
            v = dict(case=name[0], step_mode=name[1], figure="ms_per_step", parent=par, this=new, parent_median=med(par), this_median=med(new),
                     parent_spread=spread, verdict="within the parent's spread" if good else "SLOWER than the parent's spread allows")
            recs.append(v); print(json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
