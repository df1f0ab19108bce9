#!/usr/bin/env python
"""Phase stamps (egt_amd/csrc/egt_stamps.h) of one workload: per stamped kernel, mean cycles per wave and phase over every stamping wave
of every workgroup of STEPS training steps (after three warm-up steps): python tools/stamps.py narrow|attn|pair [STEPS].  Builds nothing -- run
it on a stamps build (EGT_STAMPS=1 python egt_amd/build.py --force, or tools/build_variant.sh <name> -DEGT_STAMPS for one unit + EGT_AMD_LIB=<its library>).
  narrow  a De = 8 block step (B = 64, N = 120, Dh = 64): k_narrow_fwd / k_narrow_bwd
  attn    the MFMA inner op, forward + backward (tools/bench_core.py: cfg5): k_attn_mfma_fwd / k_attn_mfma_bwd_kv
  pair    a fused-pair block step (B = 8, N = 512, Dh = 512, De = 32): k_pair_fwd / k_pair_bwd, attention and edge waves apart
The phase names come from the library (declared beside each kernel).  "waves / launch" = grid x stamping waves per workgroup.
Caveat (round 4): hipcc rotates the forward loop of k_attn_mfma_fwd -- the S MFMAs open the loop body and the P.V MFMAs follow the
barrier -- so that kernel's per-phase figures are NOT phase times (the MFMAs are not where the source has them); use the ablation
builds (-DEGT_ATTN_ABL=<bits>) for attribution and the stamps for totals."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egt_amd import egt_attention, AttnConfig, EGTBlock, _lib
from tools.bench_core import CONFIGS

dev = torch.device("cuda:0"); g = torch.Generator().manual_seed(1234)
rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)
def block_step(B, N, Dh, De, path):
    blk = EGTBlock(model_width=Dh, edge_width=De, num_heads=8, random_mask_prob=0.1).to(dev).train()
    h, e, dh, de = rnd(B, N, Dh).requires_grad_(), rnd(B, N, N, De).requires_grad_(), rnd(B, N, Dh), rnd(B, N, N, De)
    mask = torch.ones(B, N, dtype=torch.bool, device=dev)
    def step():
        h.grad = e.grad = None
        h2, e2 = blk(h, e, mask); torch.autograd.backward([h2, e2], [dh, de])
        assert blk.last_path == path, blk.last_path
    return step
def attn_step(B, N, H, d):
    qkv, E, G = rnd(B, N, 3 * d * H).requires_grad_(), rnd(B, N, N, H).requires_grad_(), rnd(B, N, N, H).requires_grad_()
    mask, dV, dH, cfg = torch.ones(B, N, dtype=torch.bool, device=dev), rnd(B, N, d * H), rnd(B, N, N, H), AttnConfig(num_heads=H)
    def step():
        qkv.grad = E.grad = G.grad = None
        V, Hh, _ = egt_attention(qkv, E, G, None, mask, cfg=cfg); torch.autograd.backward([V, Hh], [dV, dH])
    return step
def read_slots(lib):   # every slot of the library: (kernel, phase names, sums, waves); the device sums are zeroed
    out = []
    while True:
        kernel, names, n, sums, waves = C.c_char_p(), C.POINTER(C.c_char_p)(), C.c_int(), (C.c_ulonglong * 16)(), C.c_ulonglong()
        r = lib.egt_stamps_read(len(out), C.byref(kernel), C.byref(names), C.byref(n), sums, C.byref(waves))
        if r == 1: return out
        assert r == 0, "egt_stamps_read failed"
        out.append((kernel.value.decode(), [names[i].decode() if names[i] else None for i in range(n.value)], list(sums), waves.value))

step = {"narrow": lambda: block_step(64, 120, 64, 8, "fused"), "attn": lambda: attn_step(**CONFIGS["cfg5"]),
        "pair": lambda: block_step(8, 512, 512, 32, "fused-pair")}[sys.argv[1]]()
steps, lib = int(sys.argv[2]) if len(sys.argv) > 2 else 5, C.CDLL(_lib.load()._name)
if not hasattr(lib, "egt_stamps_read"): sys.exit(f"{_lib.LIB_PATH} is not a stamps build (-DEGT_STAMPS)")
for _ in range(3): step()
read_slots(lib)   # warm-up out
for _ in range(steps): step()
ran = [s for s in read_slots(lib) if s[3]]
if not ran: sys.exit("no stamped kernel ran: is the unit of this workload built with -DEGT_STAMPS?")
for kernel, names, sums, waves in ran:
    print(f"{kernel}: mean cycles per wave over {waves} waves ({steps} steps: {waves / steps:g} waves / launch), total {sum(sums) / waves:.0f}")
    for nm, s in zip(names, sums):
        if nm is not None: print(f"    {nm:42s} {s / waves:10.0f}  ({100.0 * s / sum(sums):4.1f} %)")
