"""EGT-Simple ('bias' edge channels at De = 8) on the GPU: the static-edge mode of the fused block (EGT_BF_STATIC_EDGE) at the
C boundary, block and model parity against the fp64 oracle (tests/egt_simple_ref.py composes the model loop), the autograd
route of EGTLayerStack (chained edge gradient, callers' tensors untouched), determinism, hipGraph capture and the scheme
driver on the reference's EGT-Simple configs.  Tolerances are tests/util.py's, unchanged: the fp32 forward / gradient rules,
and the bf16 rules for bf16 edge tensors."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import egt_simple_ref as R
from util import assert_close, bf16_stack_tol, BWD

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.basename(__file__)
STATIC_OFF = os.environ.get("EGT_NO_STATIC_EDGE", "") not in ("", "0")     # (child runs of this file: the route to expect)
ROUTE = "per-layer-bias" if STATIC_OFF else "static"
FWD32 = dict(rtol=2e-4, arel=5e-5)                                          # the block suites' fp32 forward rule
BF_T, BF_P = dict(rtol=2e-2, arel=1e-2, zero_atol=2e-4), dict(rtol=3e-2, arel=2e-2, l2=3e-2, zero_atol=2e-4)   # their bf16 rules

NAMES = {"attention_gates.kernel": ("attention_gates", "kernel"), "attention_gates.bias": ("attention_gates", "bias"),
         "dense_edge_b.kernel": ("dense_edge_b", "kernel"), "dense_edge_b.bias": ("dense_edge_b", "bias"),
         "norm_mha.gamma": ("norm_mha", "gamma"), "norm_mha.beta": ("norm_mha", "beta"),
         "dense_qkv.kernel": ("dense_qkv", "kernel"), "dense_qkv.bias": ("dense_qkv", "bias"),
         "dense_mha.kernel": ("dense_mha", "kernel"), "dense_mha.bias": ("dense_mha", "bias")}


def _check_grad(name, got, ref, **tol):
    """assert_close, except for d(dense_edge_b.bias): in the 'bias' variant that gradient is identically zero in exact
    arithmetic (a bias on every logit of a softmax row shifts the row; H_hat has no other consumer), so the oracle's own
    value is its rounding noise -- with an EMPTY graph in the batch every logit of that graph carries the additive -1e9 key
    mask, whose fp64 spacing 1e9 * 2^-53 = 1.1e-7 per logit puts that noise above util.assert_close's 1e-9 detector of
    analytically-zero tensors.  The premise is asserted (|oracle| < 1e-6) and the kernel's value is then held to util's
    absolute bound for such tensors (zero_atol) against exact zero."""
    if name.endswith("dense_edge_b.bias"):
        assert float(ref.abs().max()) < 1e-6, f"{name}: the oracle's value is not rounding noise"
        assert_close(got, torch.zeros_like(ref), name=name, rtol=0.0, arel=0.0, zero_atol=tol["zero_atol"])
        return
    assert_close(got, ref, name=name, **tol)


def _mha_seed(m):
    """the seed the block's next call draws its random mask from (EGT.next_seed)"""
    return (m.seed * 0x9E3779B97F4A7C15 + (m._calls + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


def _opt_in(blk):
    """what EGTLayerStack does to its 'bias' blocks (layers.py): a block on its own keeps today's route"""
    blk._static_edge, blk._static_first, blk._static_ok = True, True, {}
    return blk


def _desc(L, B, N, d=8, gated=True, clip=True, bf16=False, static=True, train=False, seed=0, p=0.0):
    flags = L.BF_NO_EDGE_LN | (L.BF_STATIC_EDGE if static else 0) | (L.BF_GATE if gated else 0) | (L.BF_CLIP if clip else 0) \
        | (L.BF_TRAINING if train else 0)
    return L.BlockDesc(B=B, N=N, H=8, d=d, De=8, dtype=L.EGT_BF16 if bf16 else L.EGT_F32, flags=flags, clip_lo=-5.0, clip_hi=5.0,
                       random_mask_prob=p, ln_eps=1e-3, reserved=0, seed=seed, seed_device=None)


# ------------------------------------------------------------------------------------------------ C-ABI contract ---
@pytest.mark.parametrize("bf16", [False, True])
def test_static_edge_c_abi_contract(bf16, gpu, egt_lib):
    """With the flag: e_out is never written (a sentinel-filled buffer stays bit for bit; NULL is accepted), the norm_edge /
    dense_edge_r pointers may be NULL, d_e may alias d_e_out (same result as separate buffers) and a NULL d_e_out equals a
    zero tensor -- torch.equal each time.  The forward equals the unflagged call with identity LayerNorm parameters and a
    zero dense_edge_r."""
    from egt_amd import _lib as L, EGTBlock
    from egt_amd.fused import _params_struct, _GRAD_ORDER
    lib = egt_lib
    B, N, Dh = 2, 37, 64
    torch.manual_seed(3)
    blk = EGTBlock(model_width=Dh, edge_width=8, edge_channel_type="bias").to(gpu)
    with torch.no_grad():
        for prm in blk.parameters():
            if prm.dim() == 1:
                prm.add_(0.2 * torch.randn_like(prm))
    edt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator().manual_seed(11)
    h = torch.randn(B, N, Dh, generator=g).to(gpu); e = (torch.randn(B, N, N, 8, generator=g) * 1.3).to(edt).to(gpu)
    dho = torch.randn(B, N, Dh, generator=g).to(gpu); deo = torch.randn(B, N, N, 8, generator=g).to(edt).to(gpu)
    km = torch.ones(B, N, dtype=torch.uint8); km[1, 30:] = 0; km = km.to(gpu)
    mods = blk._modules
    plist = [None if mod in ("norm_edge", "dense_edge_r") else mods[mod]._parameters[attr].detach().contiguous() for mod, attr in _GRAD_ORDER]
    d = _desc(L, B, N, bf16=bf16)
    assert lib.egt_block_supported(C.byref(d)) == 1
    saved = torch.empty(lib.egt_block_saved_bytes(C.byref(d)), dtype=torch.uint8, device=gpu)
    ws = torch.empty(lib.egt_block_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=gpu)
    pst = _params_struct(plist)
    st = L.current_stream()
    sentinel = torch.full_like(e, 123.0)
    keep = sentinel.clone()
    h_out = torch.empty_like(h)
    L.check(lib.egt_block_fwd(C.byref(d), C.byref(pst), L.ptr(h), L.ptr(e), L.ptr(km), None, None, L.ptr(h_out), L.ptr(sentinel),
                              L.ptr(saved), L.ptr(ws), st))
    torch.cuda.synchronize()
    assert torch.equal(sentinel.view(torch.int16 if bf16 else torch.int32), keep.view(torch.int16 if bf16 else torch.int32))
    h_out2 = torch.empty_like(h)
    L.check(lib.egt_block_fwd(C.byref(d), C.byref(pst), L.ptr(h), L.ptr(e), L.ptr(km), None, None, L.ptr(h_out2), None,
                              L.ptr(saved), L.ptr(ws), st))
    assert torch.equal(h_out, h_out2)
    # the unflagged 'bias' call: identity LN parameters, zero dense_edge_r
    d0 = _desc(L, B, N, bf16=bf16, static=False)
    full = list(plist)
    full[0], full[1], full[12], full[13] = blk._id_gamma, blk._id_beta, blk._zero_Wr, blk._zero_br
    saved0 = torch.empty_like(saved); e_out0 = torch.empty_like(e); h_out0 = torch.empty_like(h)
    pst0 = _params_struct(full)
    L.check(lib.egt_block_fwd(C.byref(d0), C.byref(pst0), L.ptr(h), L.ptr(e), L.ptr(km), None, None, L.ptr(h_out0), L.ptr(e_out0),
                              L.ptr(saved0), L.ptr(ws), st))
    assert_close(h_out, h_out0, name="h_out vs the unflagged call", rtol=1e-5, arel=1e-6)
    assert torch.equal(e_out0, e)

    def bwd(de_out, de):
        grads = [None if t is None else torch.empty_like(t) for t in plist]
        gst = _params_struct(grads)
        dh = torch.empty_like(h)
        L.check(lib.egt_block_bwd(C.byref(d), C.byref(pst), L.ptr(h), L.ptr(e), L.ptr(km), None, None, L.ptr(saved), L.ptr(dho),
                                  L.ptr(de_out), L.ptr(dh), L.ptr(de), C.byref(gst), L.ptr(ws), st))
        torch.cuda.synchronize()
        return dh, de, grads
    dh_a, de_a, g_a = bwd(deo, torch.empty_like(e))                    # separate buffers
    acc = deo.clone()
    dh_b, de_b, g_b = bwd(acc, acc)                                    # in place
    assert de_b.data_ptr() == acc.data_ptr()
    assert torch.equal(de_a, de_b) and torch.equal(dh_a, dh_b)
    for x, y in zip(g_a, g_b):
        assert (x is None and y is None) or torch.equal(x, y)
    dh_z, de_z, g_z = bwd(torch.zeros_like(e), torch.empty_like(e))    # zeros ...
    dh_n, de_n, g_n = bwd(None, torch.empty_like(e))                   # ... and NULL
    assert torch.equal(de_z, de_n) and torch.equal(dh_z, dh_n)
    for x, y in zip(g_z, g_n):
        assert (x is None and y is None) or torch.equal(x, y)
    assert float(de_n.float().abs().max()) > 0
    # the unflagged backward agrees (its LN / dense_edge_r work is on identity / zero parameters)
    grads0 = [torch.empty_like(t) for t in full]
    dh0, de0 = torch.empty_like(h), torch.empty_like(e)
    L.check(lib.egt_block_bwd(C.byref(d0), C.byref(pst0), L.ptr(h), L.ptr(e), L.ptr(km), None, None, L.ptr(saved0), L.ptr(dho),
                              L.ptr(deo), L.ptr(dh0), L.ptr(de0), C.byref(_params_struct(grads0)), L.ptr(ws), st))
    tol = dict(rtol=2e-2, arel=1e-2) if bf16 else dict(rtol=1e-4, arel=1e-5)
    assert_close(de_a.float(), de0.float(), name="de vs the unflagged call", **tol)
    assert_close(dh_a, dh0, name="dh vs the unflagged call", **tol)


def test_static_edge_supported_and_stack_refusal(gpu, egt_lib):
    from egt_amd import _lib as L
    lib = egt_lib
    sup = lambda d: lib.egt_block_supported(C.byref(d))
    assert sup(_desc(L, 4, 37)) == 1 and sup(_desc(L, 4, 37, d=6, bf16=True)) == 1
    d16 = _desc(L, 4, 37); d16.De = 16
    assert sup(d16) == 0
    dm = _desc(L, 4, 37); dm.flags |= L.BF_ATTN_MASK
    assert sup(dm) == 0
    dn = _desc(L, 4, 37); dn.flags &= ~L.BF_NO_EDGE_LN
    assert sup(dn) == 0
    prm = L.BlockParams()
    d = _desc(L, 4, 37)
    assert lib.egt_stack_fwd(C.byref(d), 2, C.byref(prm), *([None] * 9)) == L.EGT_E_FLAGS
    assert lib.egt_stack_bwd(C.byref(d), 2, C.byref(prm), *([None] * 9), C.byref(prm), None, None) == L.EGT_E_FLAGS


# --------------------------------------------------------------------------------------------------- block parity ---
# (d, N, B, gated, clip, train, bf16, launch form the default dispatch must reach)
BLOCK_CASES = [
    (8, 21, 3, True, True, True, False, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),
    (6, 37, 3, False, True, False, False, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),
    (8, 37, 3, True, False, True, False, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),
    (6, 21, 2, False, False, True, False, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),
    (8, 120, 1, True, True, True, False, "fwd=k_narrow_fwd/8w/half bwd=k_narrow_bwd/8w"),     # B = 1: eight waves, half rows
    (6, 120, 1, False, False, False, False, "fwd=k_narrow_fwd/8w/half bwd=k_narrow_bwd/8w"),
    (8, 120, 20, True, True, False, False, "fwd=k_narrow_fwd/8w bwd=k_narrow_bwd/8w"),          # 160 sixteen-row workgroups: eight waves, whole rows
    (8, 120, 33, True, True, True, False, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),           # B * ceil(N / 16) = 264 > 256: four waves at N >= 64
    (6, 37, 87, False, True, True, False, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),           # 261 workgroups
    (8, 37, 3, True, True, True, True, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),              # bf16 edge tensors
    (8, 120, 1, True, True, False, True, "fwd=k_narrow_fwd/8w/half bwd=k_narrow_bwd/8w"),
    (6, 120, 33, False, True, True, True, "fwd=k_narrow_fwd/4w bwd=k_narrow_bwd/4w"),
]


@pytest.mark.parametrize("d,N,B,gated,clip,train,bf16,form", BLOCK_CASES)
def test_bias_block_de8_vs_oracle(d, N, B, gated, clip, train, bf16, form, gpu, egt_lib):
    """One 'bias' block at De = 8 on the static-edge route: h', dh, de (= upstream + contribution) and every parameter
    gradient against the fp64 oracle; padded graphs, an empty one where the batch has room; training mode draws the
    in-kernel mask and the oracle gets the same sample (oracle/rng_ref.py)."""
    from egt_amd import EGTBlock, _lib as L
    from oracle import egt_oracle as O, rng_ref
    Dh, p = 8 * d, 0.2
    got = egt_lib.egt_block_launch_form(C.byref(_desc(L, B, N, d=d, gated=gated, clip=clip, bf16=bf16))).decode()
    assert egt_lib.egt_block_bwd_kernel(C.byref(_desc(L, B, N, d=d, gated=gated, clip=clip, bf16=bf16))) == b"k_narrow_bwd"
    fw, bw = form.split()
    assert got.startswith(fw + " ") and (bw + "/tl") in got, got
    torch.manual_seed(7 * N + d)
    blk = _opt_in(EGTBlock(model_width=Dh, edge_width=8, num_heads=8, edge_channel_type="bias", gate_attention=gated,
                           clip_logits_value=[-5, 5] if clip else None, random_mask_prob=p if train else 0.0, seed=4,
                           fused=True)).to(gpu).train(train)
    with torch.no_grad():
        for prm in blk.parameters():
            if prm.dim() == 1:
                prm.add_(0.2 * torch.randn_like(prm))
    g = torch.Generator().manual_seed(N * 5 + B)
    h = torch.randn(B, N, Dh, generator=g); e = torch.randn(B, N, N, 8, generator=g) * 1.3
    dh = torch.randn(B, N, Dh, generator=g); de = torch.randn(B, N, N, 8, generator=g)
    if bf16:
        e, de = e.bfloat16(), de.bfloat16()
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[B - 1, max(1, N - 3):] = False                          # a padded graph
    if B >= 3:
        mask[1] = False                                          # an empty one
    rm = torch.from_numpy(rng_ref.random_mask(_mha_seed(blk.mha), B, N, 8, p)) if train else None
    hg = h.to(gpu).requires_grad_(); eg = e.to(gpu).requires_grad_()
    de_up = de.to(gpu); de_keep = de_up.clone()
    h2, e2 = blk(hg, eg, mask.to(gpu))
    assert blk.last_path == "fused" and blk.last_edge_route == ROUTE
    assert e2.data_ptr() == eg.data_ptr()                        # e itself (an alias): no copy, no e' written
    torch.autograd.backward([h2, e2], [dh.to(gpu), de_up])
    assert torch.equal(de_up, de_keep), "the upstream gradient tensor was mutated"
    names = {k: v for k, v in NAMES.items() if gated or not k.startswith("attention_gates")}
    lp = {k: getattr(getattr(blk, m), a_).detach().double().cpu().requires_grad_() for k, (m, a_) in names.items()}
    h64 = h.double().requires_grad_(); e64 = e.double().requires_grad_()
    ho, eo = O.block_forward(h64, e64, mask, lp, num_heads=8, rand_mask=rm, edge_channel_type="bias", gate_attention=gated,
                             clip_logits_value=(-5.0, 5.0) if clip else None)
    assert eo is e64
    gr = torch.autograd.grad([ho], [h64, e64] + list(lp.values()), [dh.double()], allow_unused=True)
    de_ref = gr[1] + de.double()                                 # the chain: upstream + this layer's contribution
    tol, gtol, ptol = (BF_T, BF_T, BF_P) if bf16 else (FWD32, BWD, BWD)
    assert_close(h2, ho, name="h_out", **tol)
    assert_close(hg.grad, gr[0], name="dh", **gtol)
    assert_close(eg.grad.float(), de_ref, name="de", **gtol)
    for (k, (m, a_)), ref in zip(names.items(), gr[2:]):
        got_g = getattr(getattr(blk, m), a_).grad
        if ref is None:
            assert got_g is None or float(got_g.abs().max()) == 0.0, k
            continue
        _check_grad(k, got_g, ref, **ptol)


def _child(env_extra, tests, timeout=1500):
    env = dict(os.environ, **env_extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + tests,
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert " passed" in r.stdout


PARITY = [f"tests/{HERE}::test_bias_block_de8_vs_oracle", f"tests/{HERE}::test_egt_simple_models_vs_oracle",
          f"tests/{HERE}::test_static_edge_c_abi_contract"]


@pytest.mark.skipif(STATIC_OFF or os.environ.get("EGT_DEBUG_POISON_LDS", "") not in ("", "0"), reason="already a child run")
def test_parity_again_with_poisoned_lds():
    """every block / model case in a fresh process whose launches are preceded by a NaN fill of every CU's LDS (the
    'bias' instances read a narrower operand tile: nothing may depend on what the buffer held before)"""
    _child({"EGT_DEBUG_POISON_LDS": "1"}, PARITY)


@pytest.mark.skipif(STATIC_OFF or os.environ.get("EGT_DEBUG_POISON_LDS", "") not in ("", "0"), reason="already a child run")
def test_parity_again_with_the_static_route_switched_off():
    """EGT_NO_STATIC_EDGE=1 (read once per process): the same cases on the per-layer route through the residual kernels"""
    _child({"EGT_NO_STATIC_EDGE": "1"}, PARITY[:2])


# --------------------------------------------------------------------------------------------------- model parity ---
def _module_param(model, key):
    """oracle parameter name -> the module's parameter"""
    if key in ("node_emb.embeddings", "fm_emb.embeddings"):
        return getattr(model, key.split(".")[0])
    parts = key.split(".")
    if parts[0].startswith("layer"):
        ii = int(parts[0][5:])
        if parts[1] == "ffn_node":
            return getattr(model.layers.ffn_node[ii], parts[2])
        return getattr(getattr(model.layers.blocks[ii], parts[1]), parts[2])
    if parts[0].startswith("mlp_out_"):
        return getattr(model.mlp_out[int(parts[0][8:])], parts[1])
    return getattr(getattr(model, parts[0]), parts[1])


def _graphs(kind, B, N, g, sizes):
    n = torch.tensor(sizes)
    real = torch.arange(N)[None, :] < n[:, None]
    adj = (torch.rand(B, N, N, generator=g) > 0.6).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    inp = dict(graph_matrix=adj)
    if kind == "cifar10":
        nf = torch.rand(B, N, 5, generator=g); nf[~real] = -1.0
        fm = torch.where(adj > 0, torch.rand(B, N, N, generator=g), torch.tensor(-1.0))[..., None]
        inp.update(node_features=nf, feature_matrix=fm, target=torch.randint(0, 10, (B,), generator=g))
    elif kind == "pattern":
        nf = torch.randint(0, 3, (B, N), generator=g); nf[~real] = -1
        y = torch.randint(0, 2, (B, N), generator=g); y[~real] = 0
        inp.update(node_features=nf, target=y)
    else:
        nf = torch.randint(0, 28, (B, N), generator=g); nf[~real] = -1
        fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
        inp.update(node_features=nf, feature_matrix=fm, target=torch.randn(B, 1, generator=g))
    return inp


MODEL_CASES = {   # kind, model_width, edge_width, model_height, gated, edge_dtype, expected route
    "pattern": ("pattern", 64, 8, 3, True, "f32", "static"),
    "cifar10": ("cifar10", 64, 8, 2, True, "f32", "static"),
    "zinc_w64": ("zinc", 64, 8, 2, True, "f32", "static"),
    "pattern_ungated_d6": ("pattern", 48, 8, 2, False, "f32", "static"),
    "zinc_de16_fallback": ("zinc", 64, 16, 2, True, "f32", "per-layer-bias"),
    "pattern_bf16": ("pattern", 64, 8, 3, True, "bf16", "static"),
}


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_egt_simple_models_vs_oracle(case, gpu, egt_lib):
    """Predictions, loss and EVERY parameter gradient of the three model classes with edge_channel_type='bias' against the
    test-side oracle composition, in training mode (each block's in-kernel random mask reproduced by oracle/rng_ref.py).
    The edge-embedding parameters receive the chained de of all layers.  bf16 edge tensors: e is rounded once in the
    embedding and the running edge gradient once per layer -- 1 + Ly = 4 storage points, i.e. util.bf16_stack_tol(2)."""
    from egt_amd import (ZincDCTransformer, PatternDCTransformer, Cifar10DCTransformer, mae_loss, sparse_xent_loss,
                         weighted_sparse_xent_loss, class_weights_from_sizes)
    from oracle import egt_model_oracle as MO, rng_ref
    kind, Dh, De, Ly, gated, edt, route = MODEL_CASES[case]
    if STATIC_OFF and route == "static":
        route = "per-layer-bias"
    B, N, p_rm = 3, 23, 0.25
    targets = dict(zinc=1, pattern=2, cifar10=10)[kind]
    cfg = dict(model_width=Dh, edge_width=De, model_height=Ly, upto_hop=4, num_targets=targets, gate_attention=gated,
               num_node_features=3 if kind == "pattern" else 28, num_edge_features=4)
    g = torch.Generator().manual_seed(len(case) * 13 + Ly)
    inp = _graphs(kind, B, N, g, [23, 9, 17])
    params = R.init_params(kind, cfg, g)
    cls = dict(zinc=ZincDCTransformer, pattern=PatternDCTransformer, cifar10=Cifar10DCTransformer)[kind]
    model = cls(model_width=Dh, edge_width=De, model_height=Ly, upto_hop=4, edge_channel_type="bias", gate_attention=gated,
                random_mask_prob=p_rm, seed=5, edge_dtype=edt).to(gpu).train()
    with torch.no_grad():
        for k, v in params.items():
            _module_param(model, k).copy_(v)
    assert len(params) == len(model.keras_named_parameters())
    rms = [torch.from_numpy(rng_ref.random_mask(_mha_seed(blk.mha), B, N, 8, p_rm)) for blk in model.layers.blocks]
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    yo, mo = R.forward(kind, inp, p64, cfg, rand_masks=rms)
    dev = lambda k: inp[k].to(gpu)
    if kind == "zinc":
        y = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
        loss, loss_o = mae_loss(y, dev("target")), MO.mae_loss(yo, inp["target"].double())
    elif kind == "pattern":
        y, mask = model(dev("node_features"), dev("graph_matrix"), return_mask=True)
        assert torch.equal(mask.cpu(), mo)
        loss = weighted_sparse_xent_loss(y, dev("target"), mask, class_weights_from_sizes([979220, 209900], device=gpu))
        loss_o = MO.weighted_sparse_xent_loss(yo, inp["target"], mo, MO.class_weights_from_sizes([979220, 209900]))
    else:
        y = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
        loss, loss_o = sparse_xent_loss(y, dev("target")), MO.sparse_xent_loss(yo, inp["target"])
    assert model.layers.last_edge_route == route
    loss.backward()
    gro = torch.autograd.grad(loss_o, list(p64.values()), allow_unused=True)
    if edt == "bf16":
        tol, ptol = bf16_stack_tol(2), dict(bf16_stack_tol(2, params=True), zero_atol=2e-4)
    else:
        tol, ptol = FWD32, BWD
    assert_close(y, yo, name="prediction", **tol)
    assert_close(loss.reshape(1), loss_o.reshape(1), name="loss", **tol)
    checked = 0
    for k, gref in zip(p64, gro):
        prm = _module_param(model, k)
        if gref is None:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, k
            continue
        assert prm.grad is not None, k
        _check_grad(k, prm.grad, gref, **ptol); checked += 1
    assert checked == len(params)
    assert float(model.adj_emb.kernel.grad.abs().max()) > 0      # the chained de reached the edge embedding


# -------------------------------------------------------------------------- route properties: callers' tensors, determinism ---
def _stack(gpu, Ly=3, train=True, seed=2):
    from egt_amd.layers import EGTLayerStack
    torch.manual_seed(9)
    st = EGTLayerStack(model_height=Ly, model_width=64, edge_width=8, num_heads=8, edge_channel_type="bias",
                       random_mask_prob=0.1 if train else 0.0, seed=seed).to(gpu).train(train)
    return st


@pytest.mark.skipif(STATIC_OFF, reason="a property of the static route")
def test_static_route_never_mutates_a_callers_gradient(gpu, egt_lib, monkeypatch):
    """backward through a static-route stack with an explicit upstream gradient for the final e: that tensor is read, a
    fresh buffer is written; the gradient that leaves the stack carries no accumulator tag (a later backward must not
    write into it either) and equals the per-layer route's sum."""
    B, N = 2, 37
    st = _stack(gpu, train=False)
    g = torch.Generator().manual_seed(1)
    h = torch.randn(B, N, 64, generator=g).to(gpu); e = torch.randn(B, N, N, 8, generator=g).to(gpu)
    dh = torch.randn(B, N, 64, generator=g).to(gpu); de_up = torch.randn(B, N, N, 8, generator=g).to(gpu)
    keep = de_up.clone()
    mask = torch.ones(B, N, dtype=torch.bool, device=gpu)
    hg, eg = h.clone().requires_grad_(), e.clone().requires_grad_()
    h2, e2 = st(hg, eg, mask)
    assert st.last_edge_route == "static" and e2.data_ptr() == eg.data_ptr()
    torch.autograd.backward([h2, e2], [dh, de_up])
    assert torch.equal(de_up, keep)
    assert not getattr(eg.grad, "_egt_edge_acc", False) and eg.grad.data_ptr() != de_up.data_ptr()
    first = eg.grad.clone()
    # that gradient as the upstream gradient of a second backward: still only read
    hg2, eg2 = h.clone().requires_grad_(), e.clone().requires_grad_()
    h3, e3 = st(hg2, eg2, mask)
    up2 = eg.grad
    torch.autograd.backward([h3, e3], [dh, up2])
    assert torch.equal(up2, first)
    # without an upstream gradient (a readout that ignores e): the last layer takes NULL -- no zero fill -- and the three layers
    # share ONE edge-gradient buffer (allocated once, accumulated in place)
    hg3, eg3 = h.clone().requires_grad_(), e.clone().requires_grad_()
    h4, _ = st(hg3, eg3, mask)
    made = {"empty": 0, "zeros": 0}
    real_empty, real_zeros = torch.empty_like, torch.zeros_like

    def count(kind, real):
        def f(t, *a, **k):
            if tuple(t.shape) == tuple(e.shape):
                made[kind] += 1
            return real(t, *a, **k)
        return f
    monkeypatch.setattr(torch, "empty_like", count("empty", real_empty))
    monkeypatch.setattr(torch, "zeros_like", count("zeros", real_zeros))
    h4.backward(dh)
    monkeypatch.undo()
    assert made == {"empty": 1, "zeros": 0}, made
    assert_close(eg.grad, eg3.grad + de_up, name="de with / without upstream", rtol=1e-5, arel=1e-6)
    # a block called on its own behaves as before: returns the very tensor e
    blk = st.blocks[1]
    blk._static_edge = False
    try:
        _, e5 = blk(h, e, mask)
        assert e5 is e
    finally:
        blk._static_edge = True


def test_two_eager_steps_from_equal_state_are_bit_identical(gpu, egt_lib):
    from egt_amd import PatternDCTransformer
    g = torch.Generator().manual_seed(4)
    inp = _graphs("pattern", 4, 40, g, [40, 21, 33, 12])
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        m = PatternDCTransformer(model_width=64, edge_width=8, model_height=3, upto_hop=4, edge_channel_type="bias",
                                 random_mask_prob=0.1, seed=3).to(gpu).train()
        y = m(inp["node_features"].to(gpu), inp["graph_matrix"].to(gpu))
        y.square().mean().backward()
        assert m.layers.last_edge_route == ROUTE
        outs.append([y.detach().clone()] + [p.grad.clone() for p in m.keras_named_parameters().values()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_direct_gradient_sinks_on_the_static_route(gpu, egt_lib):
    """FlatGradAllReduce(direct=True): parameters whose .grad is a pre-bound view of a flat buffer receive their gradient in
    that view; the result equals the autograd-accumulated gradients."""
    from egt_amd.dp import FlatGradAllReduce
    B, N = 2, 37
    g = torch.Generator().manual_seed(2)
    h = torch.randn(B, N, 64, generator=g).to(gpu); e = torch.randn(B, N, N, 8, generator=g).to(gpu)
    mask = torch.ones(B, N, dtype=torch.bool, device=gpu)
    st = _stack(gpu, train=False)
    h2, _ = st(h.clone().requires_grad_(), e.clone().requires_grad_(), mask)
    h2.square().mean().backward()
    want = [p.grad.clone() for p in st.parameters()]
    for p in st.parameters():
        p.grad = None
    ar = FlatGradAllReduce(list(st.parameters()), direct=True)
    h3, _ = st(h.clone().requires_grad_(), e.clone().requires_grad_(), mask)
    h3.square().mean().backward()
    assert st.last_edge_route == ROUTE
    for p, w in zip(st.parameters(), want):
        assert torch.equal(p.grad, w)
    del ar


# -------------------------------------------------------------------------------------------- the scheme driver ---
def _fixture(name, **over):
    cfg = json.load(open(os.path.join(REPO, "tests", "golden", "egt_simple", name + ".json")))
    cfg.update(over)
    return cfg


def test_use_hipgraph_reproduces_the_eager_egt_simple_run(tmp_path, gpu, egt_lib):
    """the PATTERN EGT-Simple fixture config (model_height cut to 3 for the test's time) through the scheme driver: the
    hipGraph replay equals the eager run bit for bit (without the random mask the run is a deterministic function of the
    weights and the batches); with the mask it trains."""
    from egt_amd import training as T

    def run(tag, graph, p):
        torch.manual_seed(0)
        cfg = _fixture("pattern_500k_egt_simple", model_name=tag, num_epochs=2, initial_lr=2e-3, batch_size=8, model_height=3,
                       upto_hop=4, random_mask_prob=p, use_hipgraph=graph, save_path=str(tmp_path / tag))
        s = T.PatternSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
        s.execute_training(T.SyntheticPattern(64, 8, nodes=(20, 44), seed=1, pad_multiple=1),
                           T.SyntheticPattern(16, 8, nodes=(20, 44), seed=2, pad_multiple=1))
        assert s.model.layers.last_edge_route == ROUTE
        return s
    eager, graphed = run("e", False, 0.0), run("g", True, 0.0)
    assert len(graphed._graphs) >= 2
    assert [h["loss"] for h in graphed.history] == [h["loss"] for h in eager.history]
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
    r = run("r", True, 0.1)
    assert r.history[-1]["loss"] < r.history[0]["loss"]


@pytest.mark.parametrize("name", ["pattern_500k_egt_simple", "cifar10_100k_egt_simple", "cifar10_100k_egt_simple_spe"])
def test_fixture_configs_train_and_resume(name, tmp_path, gpu, egt_lib):
    """a reference EGT-Simple config, keys as shipped, on synthetic graphs: the loss falls, the checkpoint resumes"""
    from egt_amd import training as T
    cfg = _fixture(name, num_epochs=2, initial_lr=2e-3, batch_size=16, save_path=str(tmp_path / "run"))
    if name.startswith("pattern"):
        cfg["model_height"] = 4                                    # (16 layers in the config: cut for the test's time)
        cls, mk = T.PatternSVDScheme, lambda n, s: T.SyntheticPattern(n, 16, nodes=(20, 44), seed=s, pad_multiple=16)
    else:
        cls, mk = T.Cifar10SVDScheme, lambda n, s: T.SyntheticCifar10(n, 16, nodes=(20, 44), seed=s, pad_multiple=16)
    s = cls(cfg, device=gpu, print_fn=lambda *a: None)
    if cfg.get("use_svd"):
        base, nsvd = mk, s.config.num_svd_features
        mk = lambda n, sd: T.WithPositional(base(n, sd), "svd", nsvd)
    s.execute_training(mk(96, 1), mk(32, 2))
    assert s.model.layers.last_edge_route == ROUTE
    assert s.state.current_epoch == 2 and s.history[-1]["loss"] < s.history[0]["loss"], s.history
    w = np.load(tmp_path / "run" / "saved" / (cfg["model_name"] + ".npz"))
    assert "dense_edge_b_00/kernel" in w.files and not [k for k in w.files if "norm_edge" in k or "dense_edge_r" in k or "_edge_0" in k.replace("dense_edge_b", "")]
    s2 = cls(dict(cfg, num_epochs=3), device=gpu, print_fn=lambda *a: None)
    s2.load_data(mk(96, 1), mk(32, 2)); s2.load_model(); s2.load_state()
    assert s2.state.current_epoch == 2
    assert torch.equal(s2.model.layers.blocks[0].dense_qkv.kernel, s.model.layers.blocks[0].dense_qkv.kernel)
    s2.train_model()
    assert s2.state.current_epoch == 3
