"""Shared fixtures of the flat-optimizer tests (no test functions here): parameter sets, seeded gradient recipes over K steps,
the oracle -- the matching torch.optim class run in fp64 on the same fp32 gradients -- and the parity rule.

Parity rule (per tensor: a parameter, its first or its second moment):  |got - oracle| <= 4 E + 2 ulp(max |oracle|), where E is
the largest absolute deviation torch's own fp32 optimizer shows against the same fp64 run on that tensor.  The factor 4 covers
the same dozen roundings taken in another order and with fused multiply-adds; errors do not accumulate across elements.
Non-finite results must sit at exactly the elements where torch's fp32 optimizer has them, with the same values."""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

K = 5
LR = 1e-3
CLIP = 0.05
ALGOS = ("adam", "rmsprop", "sgd")
RECIPES = ("normal", "zeros", "tiny", "huge", "mixed_sign_outliers", "clipped")
SETS = ("ragged", "zinc16")
RAGGED = (1, 3, 7, 64, 2049, 4101)     # odd flat offsets, segments shorter than one vector, one longer than a work item (2048)
FACTOR = 4.0


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


@functools.lru_cache(maxsize=None)
def shapes(pset):
    if pset == "ragged":
        return tuple((n,) for n in RAGGED)
    from egt_amd import ZincDCTransformer
    model = ZincDCTransformer(model_width=16, edge_width=16, model_height=1)
    return tuple(tuple(p.shape) for p in model.trainable_parameters())


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@functools.lru_cache(maxsize=None)
def params0(pset):
    """initial parameter values (fp32, CPU): read-only, clone before use"""
    g = _gen("p", pset)
    return tuple(torch.randn(*s, generator=g) * 0.3 for s in shapes(pset))


@functools.lru_cache(maxsize=None)
def grads(pset, recipe, steps=K, tag=0):
    """[step][parameter] fp32 CPU gradients: read-only"""
    g = _gen("g", pset, recipe, tag)
    out = []
    for _ in range(steps):
        row = []
        for s in shapes(pset):
            r = torch.randn(*s, generator=g)
            sign = torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
            if recipe == "normal":
                t = r
            elif recipe == "zeros":
                t = torch.zeros(*s)
            elif recipe == "tiny":
                t = sign * 1e-18                       # squares are subnormal
            elif recipe == "huge":
                t = sign * 1e20                        # squares overflow
            elif recipe == "mixed_sign_outliers":
                t = r * torch.where(torch.rand(*s, generator=g) < 0.02, 1e4, 1e-3)
            elif recipe == "clipped":
                t = (torch.rand(*s, generator=g) * 4 - 2) * CLIP      # both sides of +-CLIP
            else:
                raise KeyError(recipe)
            row.append(t.float())
        out.append(tuple(row))
    return tuple(out)


def torch_optimizer(algo, params, lr=LR, **kw):
    """as the training driver's get_optimizer builds them"""
    if algo == "adam":
        return torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-7, **kw)
    if algo == "rmsprop":
        return torch.optim.RMSprop(params, lr=lr, alpha=0.9, eps=1e-7, **kw)
    return torch.optim.SGD(params, lr=lr, **kw)


MOMENTS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": (None, "square_avg"), "sgd": (None, None)}


def run_torch(algo, p0, gsteps, dtype, device="cpu", clip=None, lr=LR, state=None, lrs=None, **kw):
    """torch.optim over the steps of `gsteps` in `dtype`: (params, m, v, optimizer); m / v are lists or None.  The gradients are
    the fp32 values cast to `dtype`, clipped as clip_grad_value_ clips them; `state`: a state_dict() loaded before the first
    step; `lrs`: a learning rate per step."""
    ps = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in p0]
    opt = torch_optimizer(algo, ps, lr, **kw)
    if state is not None:
        opt.load_state_dict(state)
    for k, row in enumerate(gsteps):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        for p, g in zip(ps, row):
            p.grad = g.to(device=device, dtype=dtype)
        if clip is not None:
            torch.nn.utils.clip_grad_value_(ps, clip)
        opt.step()
    mk, vk = MOMENTS[algo]
    m = [opt.state[p][mk].detach() for p in ps] if mk and opt.state else None
    v = [opt.state[p][vk].detach() for p in ps] if vk and opt.state else None
    return [p.detach() for p in ps], m, v, opt


@functools.lru_cache(maxsize=None)
def oracle(algo, pset, recipe, clip):
    """fp64 on the CPU, computed once per case and shared: (params, m, v) as tuples of fp64 tensors (m / v None where the
    algorithm has none)"""
    p, m, v, _ = run_torch(algo, params0(pset), grads(pset, recipe), torch.float64, clip=CLIP if clip else None)
    return tuple(p), None if m is None else tuple(m), None if v is None else tuple(v)


def ulp(x):
    """spacing of fp32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def ratio(got, own, ref, name=""):
    """worst |got - ref| / (4 E + 2 ulp) over one tensor under the parity rule, after the non-finite elements were held to
    torch's fp32 result `own` exactly; `ref` is the fp64 oracle"""
    got, own, ref = got.detach().cpu(), own.detach().cpu(), ref.detach().cpu().double()
    assert got.dtype == torch.float32 and own.dtype == torch.float32 and got.shape == ref.shape == own.shape, name
    bad_own, bad_got = ~torch.isfinite(own), ~torch.isfinite(got)
    assert torch.equal(bad_own, bad_got), f"{name}: non-finite at {int(bad_got.sum())} elements, torch's fp32 optimizer at {int(bad_own.sum())}"
    if bool(bad_own.any()):
        a, b = got[bad_own], own[bad_own]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]), f"{name}: other non-finite values"
    ok = ~bad_own & torch.isfinite(ref)
    if not bool(ok.any()):
        return 0.0
    E = float((own.double() - ref)[ok].abs().max())
    tol = FACTOR * E + 2 * ulp(ref[ok].abs().max())
    return float((got.double() - ref)[ok].abs().max()) / tol


def worst_ratio(got, own, ref, what):
    """over the tensors of one quantity (lists in parameter order): (ratio, index)"""
    best = (0.0, -1)
    for i, (a, b, c) in enumerate(zip(got, own, ref)):
        r = ratio(a, b, c, f"{what}[{i}]")
        if r > best[0]:
            best = (r, i)
    return best


def split(flat, shp):
    """the per-parameter views of a flat buffer"""
    out, off = [], 0
    for s in shp:
        n = numel(s)
        out.append(flat[off:off + n].view(*s))
        off += n
    return out


def make_flat(p0, device, carrier_offsets=None):
    """(params, FlatGradAllReduce) on `device`; carrier_offsets: place parameter i at that float offset of ONE carrier tensor
    (returned as third value, with the (start, stop) ranges as fourth) instead of in an allocation of its own"""
    from egt_amd.dp import FlatGradAllReduce
    if carrier_offsets is None:
        ps = [torch.nn.Parameter(p.to(device).clone()) for p in p0]
        return ps, FlatGradAllReduce(ps, direct=True)
    total = carrier_offsets[-1] + p0[-1].numel() + 64
    carrier = torch.full((total,), 123.0, device=device)
    ps, ranges = [], []
    for p, off in zip(p0, carrier_offsets):
        view = carrier[off:off + p.numel()].view(*p.shape)
        view.copy_(p)
        ps.append(torch.nn.Parameter(view))
        ranges.append((off, off + p.numel()))
    return ps, FlatGradAllReduce(ps, direct=True), carrier, ranges


def run_flat(algo, p0, gsteps, device, clip=None, lr=LR, zero_grad=False, state=None, lrs=None, order=None, carrier_offsets=None):
    """FlatOptimizer over the steps: (params, m, v, optimizer, extras); `order`: a permutation of the parameters (the results
    come back in the ORIGINAL order)"""
    from egt_amd.optim import FlatOptimizer
    idx = list(range(len(p0))) if order is None else list(order)
    made = make_flat([p0[i] for i in idx], device, None if carrier_offsets is None else carrier_offsets)
    ps, flat = made[0], made[1]
    opt = FlatOptimizer(ps, flat, algo=algo, lr=lr, clip_value=clip, zero_grad=zero_grad)
    if state is not None:
        opt.load_state_dict(state)
    for k, row in enumerate(gsteps):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        for j, i in enumerate(idx):
            ps[j].grad.copy_(row[i])
        opt.step()
    shp = [tuple(p.shape) for p in ps]
    inv = [idx.index(i) for i in range(len(p0))]
    m = None if opt._m is None else [split(opt._m, shp)[j] for j in inv]
    v = None if opt._v is None else [split(opt._v, shp)[j] for j in inv]
    return [ps[j].detach() for j in inv], m, v, opt, made[2:]
