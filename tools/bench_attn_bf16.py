#!/usr/bin/env python3
"""The MFMA inner op with bf16 products (EGT_ATTN_MM_BF16) against its exact fp32 default, at core-op scope, measured in one visit;
every measurement is a FRESH child process under its own time limit, and the first child that fails ends the run.

    python tools/bench_attn_bf16.py --parent-tree PARENT [--rounds 3] [--out profiles/attn_bf16.jsonl]

A step is egt_attn_mfma_fwd + egt_attn_mfma_bwd through the C ABI with the shared workspace (gated, edge bias, key mask, clip,
training with the in-kernel random mask at p = 0.1: the straight-line instances, what bench.py's synthetic_n512 runs).
Shapes: [8, 512] d = 64 (BASELINE config 5), [32, 512] d = 64, [8, 512] d = 16 and d = 32.
Arms: this tree in fp32 mode, this tree in bf16 mode, the parent tree in fp32 mode (the guard), alternating over --rounds.
Per child: median ms per step over --steps timed steps, then the launch profiler's mean microseconds per kernel.
Derived per record: the fraction of 8 TB/s the op's algorithmic HBM bytes imply (E, G, H_hat in the forward; E, G, dH, dE, dG and
the dA hand-off (fp32 tiles, bf16 tiles in bf16 mode), written and read, in the backward; qkv / V_att / their gradients and the operand copies on top), and the
fractions of both matrix roofs (157.3 TF fp32, 2516.8 TF bf16) at 12 N^2 d H FLOP per graph and step.
Verdicts: per case, the bf16 arm against the fp32 arm's own spread (max - min over its rounds); the guard: this tree's fp32 arm
against the parent's spread.  Output: one JSON line per measurement, then the verdict lines; exit status 1 if the guard fails."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MM_BF16 = 0x2        # EGT_ATTN_MM_BF16 (a literal: the child also runs in the parent tree, whose mirror lacks the name)
H = 8
CASES = [(8, 512, 64), (32, 512, 64), (8, 512, 16), (8, 512, 32)]
KERNELS = {"f32": ("k_attn_pack", "k_attn_mfma_fwd", "k_attn_mfma_bwd_kv", "k_attn_mfma_bwd_q"),
           "bf16": ("k_attn_bf16_pack", "k_attn_bf16_fwd", "k_attn_bf16_bwd_kv", "k_attn_bf16_bwd_q")}
HBM, ROOF_F32, ROOF_BF16 = 8.0e12, 157.3e12, 2516.8e12


def hbm_bytes(B, N, d, mode):
    pair = B * N * N * H * 4                      # one [B,N,N,H] fp32 tensor
    node = B * N * d * H * 4
    dA = pair if mode == "f32" else pair // 2     # the dA hand-off: fp32 tiles, bf16 tiles in bf16 mode
    fwd = 3 * pair + 3 * node + node + 2 * 3 * node            # E, G, H_hat; qkv in, V_att out; three operand copies written and read
    bwd = 5 * pair + 2 * dA + (3 + 1 + 1 + 3) * node + 2 * 3 * node   # E, G, dH, dE, dG; dA written and read
    return fwd, bwd


def child(args):
    sys.path.insert(0, os.getcwd())      # the tree this child was started in
    import torch
    from egt_amd import _lib as L
    from egt_amd.functional import AttnConfig, _attn_desc
    lib = L.load()
    B, N, d = args.B, args.N, args.d
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    qkv, E, G, dV, dH = r(B, N, 3 * d * H) * 0.7, r(B, N, N, H), r(B, N, N, H), r(B, N, d * H), r(B, N, N, H)
    km = torch.ones(B, N, dtype=torch.uint8, device=dev)
    desc = _attn_desc(AttnConfig(random_mask_prob=0.1, training=True, seed=7), B, N, d, True, True, False)
    desc.reserved = L.ATTN_WS_SHARED | (MM_BF16 if args.mode == "bf16" else 0)
    p = C.byref(desc)
    ws = torch.empty(lib.egt_attn_mfma_workspace_bytes(p), dtype=torch.uint8, device=dev)
    v_att, h_hat, rs = torch.empty(B, N, d * H, device=dev), torch.empty(B, N, N, H, device=dev), torch.empty(B, N, H, 4, device=dev)
    d_qkv, d_E, d_G = torch.empty_like(qkv), torch.empty_like(E), torch.empty_like(G)
    st = L.current_stream()

    def step():
        L.check(lib.egt_attn_mfma_fwd(p, L.ptr(qkv), L.ptr(E), L.ptr(G), L.ptr(km), None, None, L.ptr(v_att), L.ptr(h_hat), L.ptr(rs),
                                      L.ptr(ws), st))
        L.check(lib.egt_attn_mfma_bwd(p, L.ptr(qkv), L.ptr(E), L.ptr(G), L.ptr(km), None, None, L.ptr(v_att), L.ptr(rs), L.ptr(dV),
                                      L.ptr(dH), L.ptr(d_qkv), L.ptr(d_E), L.ptr(d_G), L.ptr(ws), st))
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    rec = dict(B=B, N=N, d=d, mode=args.mode, steps=args.steps, ms_per_step=statistics.median(ts), steps_ms=ts,
               workspace_bytes=ws.numel())
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    lib.egt_prof_enable(0)
    ks = {}
    for nm in KERNELS[args.mode]:
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(nm.encode(), C.byref(cnt), C.byref(ms))
        if cnt.value:
            ks[nm] = dict(launches=cnt.value, us_per_launch=round(ms.value / cnt.value * 1e3, 2))
    rec["kernels"] = ks
    kernel_us = sum(k["us_per_launch"] * k["launches"] / 5 for k in ks.values())
    fwd_b, bwd_b = hbm_bytes(B, N, d, args.mode)
    flop = 12.0 * N * N * d * H * B
    rec.update(kernel_us_per_step=round(kernel_us, 1), hbm_bytes=[fwd_b, bwd_b],
               hbm_frac_of_8TBs=round((fwd_b + bwd_b) / (kernel_us * 1e-6) / HBM, 3),
               frac_fp32_matrix_roof=round(flop / (kernel_us * 1e-6) / ROOF_F32, 3),
               frac_bf16_matrix_roof=round(flop / (kernel_us * 1e-6) / ROOF_BF16, 4))
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_bf16.jsonl"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--child", action="store_true", help="(internal)")
    ap.add_argument("--mode", default="f32"); ap.add_argument("--B", type=int); ap.add_argument("--N", type=int); ap.add_argument("--d", type=int)
    args = ap.parse_args()
    if args.child:
        return child(args)
    me, recs = os.path.abspath(__file__), []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = open(args.out, "w")

    def emit(o):               # kept as it comes: a child that fails later loses nothing measured before it
        recs.append(o)
        print(json.dumps({k: v for k, v in o.items() if k != "steps_ms"}), flush=True)
        sink.write(json.dumps(o) + "\n"); sink.flush()

    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    arms = [(REPO, "this", "f32"), (REPO, "this", "bf16")] + ([(parent, "parent", "f32")] if parent else [])
    for rnd in range(args.rounds):
        for B, N, d in CASES:
            for tree, tag, mode in arms:
                env = dict(os.environ)
                env.pop("EGT_AMD_LIB", None)
                cmd = [sys.executable, me, "--child", "--mode", mode, "--B", str(B), "--N", str(N), "--d", str(d),
                       "--steps", str(args.steps), "--warmup", str(args.warmup)]
                r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                if r.returncode != 0:      # a failed child ends the run: nothing more is started on the GPU
                    sys.stderr.write((r.stdout + r.stderr)[-3000:])
                    raise SystemExit(f"child {tag}/{mode} [{B},{N}] d={d} failed with exit status {r.returncode}; nothing more is run")
                for line in r.stdout.splitlines():
                    if line.startswith("RESULT "):
                        emit(dict(json.loads(line[7:]), tree=tag, round=rnd))
    med = lambda v: sorted(v)[len(v) // 2]
    ok = True
    for B, N, d in CASES:
        sel = lambda t, m: [r["ms_per_step"] for r in recs if (r.get("B"), r.get("N"), r.get("d"), r.get("tree"), r.get("mode")) == (B, N, d, t, m)]
        f32, bf, par = sel("this", "f32"), sel("this", "bf16"), sel("parent", "f32")
        spread = max(f32) - min(f32)
        gain = med(f32) - med(bf)
        emit(dict(case=[B, N, d], figure="ms_per_step", f32=f32, bf16=bf, f32_median=med(f32), bf16_median=med(bf), f32_spread=spread,
                  speedup=round(med(f32) / med(bf), 3),
                  verdict="bf16 faster outside the fp32 arm's spread" if gain > spread else
                          "bf16 SLOWER outside the fp32 arm's spread" if -gain > spread else "no difference outside the fp32 arm's spread"))
        if par:
            ps = max(par) - min(par)
            good = med(f32) <= med(par) + ps
            ok &= good
            emit(dict(case=[B, N, d], guard="this tree fp32 vs parent fp32", parent=par, this=f32, parent_median=med(par), this_median=med(f32),
                      parent_spread=ps, verdict="within the parent's spread" if good else "SLOWER than the parent's spread allows"))
    sink.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
