#!/usr/bin/env python3
"""Randomised parity sweep of the fused stack (and FFN) against the fp64 oracle over edge-case
geometries.  Test infrastructure (imports oracle/): run on the GPU box, prints failures.
--recipe NAME applies one conditioning recipe of tests/conditioning.py to the random cases (stack: the data recipes, pad32,
gates_sat, small_weights; inner op: sharp, gates_sat, edge_bias_big; FFN: the data recipes and small_weights); the outputs that
contain a residual input are then compared as updates out - in, at the sweep's own tolerances.  Without it nothing changes.
A recipe that does not apply to a part of the sweep leaves that part as it is, and main() says so.  gates_sat is not applied to
inner-op configurations with N <= 3: with so few keys no gate may be left unsaturated, and the fp32 sigmoid's 1 - g == 0 then reads as
a dG failure although a plain fp32 evaluation does the same (the recipes' strengths are held fair only on the cases of
tests/test_conditioning_cpu.py)."""
import itertools
import os
import random
import sys
import traceback

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from util import assert_close, BWD  # noqa: E402
from test_block_gpu import PMAP  # noqa: E402


DATA_RECIPES = ("offset32", "const_rows", "tiny", "big", "outliers")
STACK_RECIPES = DATA_RECIPES + ("pad32", "gates_sat", "small_weights")
ATTN_RECIPES = ("sharp", "gates_sat", "edge_bias_big")
FFN_RECIPES = DATA_RECIPES + ("small_weights",)


def one(N, De, d, gated, train, Ly, B, dev, seed, recipe=None):
    from egt_amd import EGTStack
    from egt_amd.fused import layer_seed
    from oracle import egt_oracle as O, rng_ref
    Dh, p = 8 * d, 0.25
    if recipe not in STACK_RECIPES:
        recipe = None
    torch.manual_seed(seed)
    st = EGTStack(model_height=Ly, model_width=Dh, edge_width=De, num_heads=8, gate_attention=gated,
                  random_mask_prob=p if train else 0.0, seed=seed, fused=True).to(dev).train(train)
    with torch.no_grad():
        for prm in st.parameters():
            if prm.dim() == 1:
                prm.add_(0.2 * torch.randn_like(prm))
    g = torch.Generator().manual_seed(seed + 1)
    h = torch.randn(B, N, Dh, generator=g); e = torch.randn(B, N, N, De, generator=g) * 1.3
    mask = torch.ones(B, N, dtype=torch.bool)
    if N > 2:
        mask[B - 1, N - max(1, N // 4):] = False
    dh = torch.randn(B, N, Dh, generator=g); de = torch.randn(B, N, N, De, generator=g)
    if recipe in STACK_RECIPES:
        import conditioning as CD
        gr_, s_ = CD.gen("sweep", seed, recipe), CD.strength("stack", recipe)
        if recipe in DATA_RECIPES:
            h, e = CD.condition(h, recipe, gr_, s_), CD.condition(e, recipe, gr_, s_)
        elif recipe == "pad32":
            node, pair = CD.pad_regions(mask)
            h, e = CD.pad32(h, node, gr_, s_), CD.pad32(e, pair, gr_, s_)
        else:
            with torch.no_grad():
                for blk in st.blocks:
                    for m in (["attention_gates"] if recipe == "gates_sat" else [m for m, a_ in PMAP.values() if a_ == "kernel"]):
                        if hasattr(blk, m) and (gated or m != "attention_gates"):
                            getattr(blk, m).kernel.mul_(s_)
    hg = h.to(dev).requires_grad_(); eg = e.to(dev).requires_grad_()
    h2, e2 = st(hg, eg, mask.to(dev))
    assert st.last_path == "fused-stack", st.last_path
    torch.autograd.backward([h2, e2], [dh.to(dev), de.to(dev)])
    names = {k: v for k, v in PMAP.items() if gated or not k.startswith("attention_gates")}
    layers = [{k: getattr(getattr(blk, m), a_).detach().double().cpu().requires_grad_()
               for k, (m, a_) in names.items()} for blk in st.blocks]
    rms = None
    if train:
        b0 = st.blocks[0].mha
        sd = (b0.seed * 0x9E3779B97F4A7C15 + b0._calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        rms = [torch.from_numpy(rng_ref.random_mask(layer_seed(sd, l), B, N, 8, p)) for l in range(Ly)]
    h64 = h.double().requires_grad_(); e64 = e.double().requires_grad_()
    ho, eo = O.stack_forward(h64, e64, mask, layers, num_heads=8, rand_masks=rms, gate_attention=gated)
    flat = [t for lp in layers for t in lp.values()]
    gr = torch.autograd.grad([ho, eo], [h64, e64] + flat, [dh.double(), de.double()])
    if recipe is None:
        assert_close(h2, ho, name="h_out", rtol=2e-4, arel=5e-5)
        assert_close(e2, eo, name="e_out", rtol=2e-4, arel=5e-5)
    else:        # the updates: the whole-tensor maximum of h' / e' would loosen every element by the offset / the padding
        regions = [("", None, None)]
        if recipe == "pad32":
            node, pair = CD.pad_regions(mask)
            regions = [("[real]", node, pair), ("[pad]", ~node, ~pair)]
        for tag, node, pair in regions:
            for name, out, ref, base, idx in (("h_out", h2, ho, h, node), ("e_out", e2, eo, e, pair)):
                a, r, b = out.detach().double().cpu(), ref.detach(), base.double()
                if tag != "[pad]":
                    a, r = a - b, r - b
                if idx is not None:
                    a, r = a[idx], r[idx]
                if a.numel():
                    assert_close(a, r, name=name + tag, rtol=2e-4, arel=5e-5)
    assert_close(hg.grad, gr[0], name="dh", **BWD)
    assert_close(eg.grad, gr[1], name="de", **BWD)
    gi = iter(gr[2:])
    for li, blk in enumerate(st.blocks):
        for k, (m, a_) in names.items():
            assert_close(getattr(getattr(blk, m), a_).grad, next(gi), name=f"L{li}.{k}", **BWD)


def one_ffn(shape, act, dev, seed, W, recipe):
    """test_ffn_gpu._run with a conditioning recipe on x (or the two kernels); y compared as the update y - x"""
    import conditioning as CD
    from egt_amd import FFN
    from oracle import egt_oracle as O
    from util import FWD
    NAMES = CD.FFN_NAMES
    torch.manual_seed(seed)
    m = FFN(W, activation=act).to(dev)
    with torch.no_grad():
        for n in ("norm_gamma", "norm_beta", "lr1_bias", "lr2_bias"):
            getattr(m, n).add_(0.3 * torch.randn_like(getattr(m, n)))
        if recipe == "small_weights":
            m.lr1_kernel.mul_(CD.strength("ffn", recipe)); m.lr2_kernel.mul_(CD.strength("ffn", recipe))
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(*shape, W, generator=g) * 1.5 + 0.2
    dy = torch.randn(*shape, W, generator=g)
    x = CD.condition(x, recipe, CD.gen("sweep-ffn", seed, recipe), CD.strength("ffn", recipe))
    xg = x.to(dev).requires_grad_()
    y = m(xg)
    y.backward(dy.to(dev))
    p64 = {n: getattr(m, n).detach().double().cpu().requires_grad_() for n in NAMES}
    x64 = x.double().requires_grad_()
    yo = O.ffn_forward(x64, p64, activation=act)
    gr = torch.autograd.grad(yo, [x64] + [p64[n] for n in NAMES], dy.double())
    assert_close(y.detach().double().cpu() - x.double(), yo.detach() - x.double(), name="y (update)", **FWD)
    assert_close(xg.grad, gr[0], name="dx", **BWD)
    for n, gref in zip(NAMES, gr[1:]):
        assert_close(getattr(m, n).grad, gref, name="d" + n, **BWD)


def one_attn(N, d, opts, B, dev, seed, recipe=None):
    """inner op through the C-ABI (general kernels, and the MFMA path when d in {16,32,64}) vs the oracle"""
    import cases as CS
    from test_attn_gpu import run_hip, compare
    H = 8
    g = torch.Generator().manual_seed(seed)
    QKV = torch.randn(B, N, 3 * d * H, generator=g) * 0.8
    E = torch.randn(B, N, N, H, generator=g) if opts["edge"] else None
    G = torch.randn(B, N, N, H, generator=g) if opts["gate"] else None
    M = None
    if opts["attn_mask"]:
        M = (torch.rand(B, N, N, generator=g) > 0.4).float()[..., None].repeat(1, 1, 1, H).contiguous()
    mask = None
    if opts["pad"]:
        mask = torch.ones(B, N, dtype=torch.bool)
        mask[B - 1, N - max(1, N // 3):] = False
    rm = (torch.rand(B, N, N, H, generator=g) < 0.3) if opts["rand"] else None
    pd = 0.2 if opts["drop"] else 0.0
    dk = (torch.rand(B, N, N, H, generator=g) >= pd) if opts["drop"] else None
    inp = dict(QKV=QKV, E=E, G=G, M=M, mask=mask, rand_mask=rm, drop_keep=dk,
               dV=torch.randn(B, N, d * H, generator=g), dH=torch.randn(B, N, N, H, generator=g))
    if recipe in ATTN_RECIPES and not (recipe == "gates_sat" and N <= 3):
        import conditioning as CD
        s_ = CD.strength("attn", recipe)
        if recipe == "sharp":
            inp["QKV"] = inp["QKV"] * s_
        elif recipe == "gates_sat" and G is not None:
            inp["G"] = G * s_
        elif recipe == "edge_bias_big" and E is not None:
            inp["E"], opts = E * s_, dict(opts, clip=False)
    attrs = dict(num_heads=H, clip_logits_value=(-5.0, 5.0) if opts["clip"] else None,
                 scale_degree=opts["deg"] and opts["gate"], scaler_type=opts["scaler"],
                 num_virtual_nodes=1 if (opts["deg"] and N > 2) else 0, attn_dropout=pd)
    compare(run_hip(inp, attrs, dev, a_tild=opts["atild"]) if opts["atild"] else
            {**run_hip(inp, attrs, dev, a_tild=False), "A_tild": CS.attn_oracle(inp, attrs)["A_tild"]},
            CS.attn_oracle(inp, attrs))


def main(seed=None, n_stack=None, n_attn=70, n_ffn=24, recipe=None):
    dev = torch.device("cuda", 0)
    import os
    if seed is None:
        seed = int(os.environ.get("EGT_SWEEP_SEED", "2024"))   # other seeds: other geometries / feature mixes
    rnd = random.Random(seed)
    if recipe is not None:
        for part, known in (("stack", STACK_RECIPES), ("inner op", ATTN_RECIPES), ("FFN", FFN_RECIPES)):
            if recipe not in known:
                print(f"sweep: --recipe {recipe} has no effect on the {part} cases (they run unconditioned)")
    Ns = [1, 2, 3, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 80]
    if seed != 2024:
        Ns = sorted(rnd.sample(range(1, 161), 16))
    combos = []
    for N in Ns:
        for _ in range(3):
            combos.append((N, rnd.choice([8, 16, 32, 48, 64]), rnd.choice([1, 2, 3, 4, 5, 6, 7, 8]),
                           rnd.random() < 0.8, rnd.random() < 0.5, rnd.choice([1, 2, 3]), rnd.choice([1, 2, 5])))
    combos += [(64, 64, 8, True, True, 3, 4), (64, 64, 8, False, False, 2, 3), (128, 64, 8, True, True, 1, 2),
               (16, 64, 8, True, False, 2, 1), (96, 16, 8, True, True, 2, 2)]
    if n_stack is not None:
        combos = combos[:n_stack]
    bad = 0
    for i, (N, De, d, gated, train, Ly, B) in enumerate(combos):
        try:
            one(N, De, d, gated, train, Ly, B, dev, seed=100 + i, recipe=recipe)
        except Exception as ex:  # noqa: BLE001
            bad += 1
            print("FAIL", dict(N=N, De=De, d=d, gated=gated, train=train, Ly=Ly, B=B), type(ex).__name__, str(ex)[:300])
            if not isinstance(ex, AssertionError):
                traceback.print_exc()
    print(f"sweep: {len(combos) - bad}/{len(combos)} geometries ok")
    nat = 0
    for i in range(n_attn):
        N = rnd.choice([1, 2, 3, 5, 15, 16, 17, 33, 48, 63, 64, 70])
        d = rnd.choice([1, 2, 3, 5, 8, 8, 16, 32, 64])
        opts = dict(edge=rnd.random() < 0.8, gate=rnd.random() < 0.7, attn_mask=rnd.random() < 0.3,
                    pad=rnd.random() < 0.7, rand=rnd.random() < 0.5, drop=rnd.random() < 0.25,
                    clip=rnd.random() < 0.8, deg=rnd.random() < 0.25, scaler=rnd.choice(["log", "linear"]),
                    atild=rnd.random() < 0.5)
        nat += 1
        try:
            one_attn(N, d, opts, rnd.choice([1, 2, 3]), dev, seed=500 + i, recipe=recipe)
        except Exception as ex:  # noqa: BLE001
            bad += 1
            print("FAIL attn", dict(N=N, d=d, **opts), type(ex).__name__, str(ex)[:300])
            if not isinstance(ex, AssertionError):
                traceback.print_exc()
    print(f"sweep: inner op {nat} random configurations done, total failures {bad}")
    # channel FFN: random row counts / widths / activations
    from test_ffn_gpu import _run as ffn_run
    nf = 0
    for i in range(n_ffn):
        W = rnd.choice([16, 32, 48, 64])
        shape = rnd.choice([(1,), (rnd.randint(1, 70),), (rnd.randint(1, 5), rnd.randint(1, 40)),
                            (rnd.randint(1, 3), rnd.randint(2, 33), rnd.randint(2, 33))])
        if len(shape) == 3:
            shape = (shape[0], shape[1], shape[1])
        nf += 1
        try:
            if recipe in FFN_RECIPES:
                one_ffn(shape, rnd.choice(["elu", "relu"]), dev, seed=900 + i, W=W, recipe=recipe)
            else:
                ffn_run(shape, rnd.choice(["elu", "relu"]), dev, seed=900 + i, W=W)
        except Exception as ex:  # noqa: BLE001
            bad += 1
            print("FAIL ffn", dict(W=W, shape=shape), type(ex).__name__, str(ex)[:300])
            if not isinstance(ex, AssertionError):
                traceback.print_exc()
    print(f"sweep: FFN {nf} random shapes done, total failures {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--recipe", default=None, choices=sorted(set(STACK_RECIPES + ATTN_RECIPES + FFN_RECIPES)),
                    help="apply one conditioning recipe (tests/conditioning.py) to the random cases")
    sys.exit(main(recipe=ap.parse_args().recipe))
