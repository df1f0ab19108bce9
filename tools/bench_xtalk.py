#!/usr/bin/env python3
"""Cross-talk FFN (node2edge_xtalk / edge2node_xtalk), measured in one visit; every measurement is a FRESH child process under its
own time limit, and the first child that fails ends the run.

    python tools/bench_xtalk.py [--parent-tree PARENT] [--rounds 3] [--out profiles/xtalk.jsonl]

  (a) one layer's FFN pair with cross-talk at [128, 64, 64, 64] (Dh 64) and [128, 37, 37, 48 -> De 32] -- see SHAPES --, fractions
      .25 / .25, forward + backward: the fused op (egt_amd.xtalk.xtalk_ffn) against xtalk_ffn_composed, alternating over --rounds,
      median of --steps timed steps each.  The fused child also records its kernels per launch (the library's launch profiler) and
      the fraction of 8 TB/s that the algorithmic HBM bytes of k_xtalk_fwd (e read, e' written) and k_xtalk_bwd (e and d e' read,
      d e written) imply.
  (b) the ZINC-500K model step (10 layers, width 64, N = 64, B = 128, random_mask_prob 0.1) with both keys at .25, both routes.
  (c) the guard: the same step with the keys off and the headline bench.py line, this tree against --parent-tree (a built checkout
      of the parent commit), alternating over --rounds; the verdict per case against the parent's own spread (max - min over its
      rounds).
Output: one JSON line per measurement, then the comparison / verdict lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# B, N, Dh, De.  The second shape is the ZINC-100K batch geometry (N = 37, node width 48); its edge width 48 is outside what the
# kernels cover (De 16 / 32 / 64), so it runs at De = 32
SHAPES = {"n64_de64": (128, 64, 64, 64), "n37_dh48_de32": (128, 37, 48, 32)}
FRAC = 0.25
HBM = 8.0e12
KERNELS = ("k_xtalk_prep", "k_xtalk_fwd", "k_xtalk_bwd", "k_xtalk_colsum", "k_xtalk_sum", "k_xtalk_param_grads")


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


def child_op(args, shape, fused):
    sys.path.insert(0, os.getcwd())
    import torch
    from egt_amd import _lib, xtalk as XT
    lib = _lib.load()
    B, N, Dh, De = SHAPES[shape]
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    kn, ke = XT.lr2_widths(De, Dh, FRAC, FRAC)
    pn, pe = XT.XtalkFFNParams(Dh, kn).to(dev), XT.XtalkFFNParams(De, ke).to(dev)
    h = torch.randn(B, N, Dh, generator=g).to(dev).requires_grad_()
    e = torch.randn(B, N, N, De, generator=g).to(dev).requires_grad_()
    n = torch.randint(int(0.6 * N), N + 1, (B,), generator=g); n[0] = N
    mask = (torch.arange(N)[None, :] < n[:, None]).to(dev)
    dh, de = torch.randn_like(h), torch.randn_like(e)
    op = XT.xtalk_ffn if fused else XT.xtalk_ffn_composed

    def fn():
        h.grad = e.grad = None
        h2, e2 = op(h, e, mask, pn.tensors(), pe.tensors(), FRAC, FRAC, "elu")
        torch.autograd.backward([h2, e2], [dh, de])
    ms, ts = _timed(fn, args.steps, args.warmup)
    rec = dict(case="xtalk_ffn", shape=shape, B=B, N=N, Dh=Dh, De=De, fractions=[FRAC, FRAC], steps=args.steps, ms_per_step=ms, steps_ms=ts)
    if fused:
        lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        lib.egt_prof_enable(0)
        ks = {}
        for nm in KERNELS:
            cnt, t = C.c_int64(0), C.c_double(0.0)
            lib.egt_prof_read(nm.encode(), C.byref(cnt), C.byref(t))
            if cnt.value:
                ks[nm] = dict(launches=cnt.value, us_per_launch=round(t.value / cnt.value * 1e3, 2))
        rec["kernels"] = ks
        tensor = B * N * N * De * 4
        for nm, nbytes in (("k_xtalk_fwd", 2 * tensor), ("k_xtalk_bwd", 3 * tensor)):
            if nm in ks:
                ks[nm]["hbm_bytes"] = nbytes
                ks[nm]["hbm_fraction"] = round(nbytes / (ks[nm]["us_per_launch"] * 1e-6) / HBM, 3)
    print("RESULT " + json.dumps(rec), flush=True)


def child_model(args, on, fused=True):
    sys.path.insert(0, os.getcwd())
    import torch
    from egt_amd import ZincDCTransformer, mae_loss
    from egt_amd.dp import FlatGradAllReduce
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
    torch.manual_seed(0)
    kw = dict(node2edge_xtalk=FRAC, edge2node_xtalk=FRAC) if on else {}      # (off: the parent's keywords only)
    model = ZincDCTransformer(model_width=64, edge_width=64, model_height=10, num_heads=8, upto_hop=16, random_mask_prob=0.1, seed=1,
                              **kw).to(dev).train()
    if on:
        model.layers.xtalk_fused = fused
    flat = FlatGradAllReduce(model.trainable_parameters(), direct=True)

    def fn():
        flat.zero(); flat.rebind()
        loss = mae_loss(model(*inputs), y)
        loss.backward()
        return loss.detach()
    ms, ts = _timed(fn, args.steps, args.warmup)
    print("RESULT " + json.dumps(dict(case="zinc500k_model_step", xtalk=[FRAC, FRAC] if on else [0, 0], B=B, N=N, layers=10, steps=args.steps,
                                      xtalk_route=getattr(model.layers, "last_xtalk_route", None), ms_per_step=ms, steps_ms=ts,
                                      graphs_per_s=B / ms * 1e3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "xtalk.jsonl"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--child", default=None, help="(internal) op:<shape>:<fused|composed> | model:on:<fused|composed> | model:off")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--skip", default="", help="comma list of a, b, c")
    args = ap.parse_args()
    if args.child:
        kind, what, *arm = args.child.split(":")
        fused = not arm or arm[0] == "fused"
        return child_op(args, what, fused) if kind == "op" else child_model(args, what == "on", fused)
    me, recs, skip = os.path.abspath(__file__), [], set(args.skip.split(","))

    def run(cmd, tree, tag):
        env = dict(os.environ)
        env.pop("EGT_AMD_LIB", None)
        r = subprocess.run([sys.executable] + cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:      # a failed child ends the run: nothing more is started on the GPU
            sys.stderr.write((r.stdout + r.stderr)[-3000:])
            raise SystemExit(f"child {cmd[1:]} ({tag}) failed with exit status {r.returncode}; nothing more is run")
        for line in r.stdout.splitlines():
            o = None
            if line.startswith("RESULT "):
                o = dict(json.loads(line[7:]), **tag)
            elif line.startswith("{") and "ms_per_step" in line:      # bench.py's result line
                d = json.loads(line)
                o = dict(case="bench.py headline", ms_per_step=d["ms_per_step"], median_ms_per_step=d.get("median_ms_per_step"),
                         value=d.get("value"), metric=d.get("metric"), **tag)
            if o is not None:
                recs.append(o)
                print(json.dumps({k: v for k, v in o.items() if k != "steps_ms"}), flush=True)

    common = ["--steps", str(args.steps), "--warmup", str(args.warmup)]
    med = lambda v: sorted(v)[len(v) // 2]
    ok = True
    for rnd in range(args.rounds):
        for route in ("fused", "composed"):
            if "a" not in skip:
                for shape in SHAPES:
                    run([me, "--child", f"op:{shape}:{route}"] + common, REPO, dict(part="a", arm=route, round=rnd))
            if "b" not in skip:
                run([me, "--child", f"model:on:{route}"] + common, REPO, dict(part="b", arm=route, round=rnd))
    for part, key in (("a", "shape"), ("b", "case")):
        runs = [r for r in recs if r.get("part") == part]
        for k in dict.fromkeys(r[key] for r in runs):
            sel = lambda arm: [r["ms_per_step"] for r in runs if r[key] == k and r["arm"] == arm]
            fu, co = sel("fused"), sel("composed")
            spread = max(co) - min(co)
            good = med(fu) <= med(co) + spread
            ok &= good
            v = dict(compare=part, key=k, figure="ms_per_step", fused=fu, composed=co, fused_median=med(fu), composed_median=med(co),
                     composed_spread=spread, speedup=round(med(co) / med(fu), 3),
                     verdict="fused no slower than composed" if good else "fused SLOWER than composed")
            recs.append(v); print(json.dumps(v), flush=True)
    if "c" not in skip:
        trees = ([(os.path.abspath(args.parent_tree), "parent")] if args.parent_tree else []) + [(REPO, "this")]
        for rnd in range(args.rounds):
            for tree, tag in trees:
                run([me, "--child", "model:off"] + common, tree, dict(part="c", tree=tag, round=rnd))
                run(["bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "10", "--no-cpu-baseline"], tree, dict(part="c", tree=tag, round=rnd))
        runs = [r for r in recs if r.get("part") == "c"]
        for name in dict.fromkeys(r["case"] for r in runs):
            sel = lambda t: [r["ms_per_step"] for r in runs if r["case"] == name and r["tree"] == t]
            par, new = sel("parent"), sel("this")
            if not par:
                continue
            spread = max(par) - min(par)
            good = med(new) <= med(par) + spread
            ok &= good
            v = dict(case=name, figure="ms_per_step", parent=par, this=new, parent_median=med(par), this_median=med(new),
                     parent_spread=spread, verdict="within the parent's spread" if good else "SLOWER than the parent's spread allows")
            recs.append(v); print(json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
