"""The host path around the fused block, pinned without a GPU: a block call is the one-layer stack call (buffer sizes), the
argument errors of egt_block_* / egt_stack_* (code and message, all answered before any launch), the route table of
egt_amd.fused.route_core, and the memo of the library's coverage answers.  ROUTE_CASES is shared with tests/test_route_gpu.py,
which runs the same configurations for real; the expected routes and error strings were recorded from the predicates and the
library of the commit before the host path was unified."""
import ctypes as C

import pytest
import torch

from test_block_plan_cpu import cases


# ------------------------------------------------------------------------------------------- block = one-layer stack ---
def test_block_is_the_one_layer_stack(egt_lib):
    from egt_amd import _lib as L
    n = 0
    for name, B, N, d, De, bf, ml in cases():
        flags = L.BF_GATE | L.BF_CLIP | L.BF_TRAINING | (L.BF_ATTN_MASK if ml else 0)
        desc = L.BlockDesc(B=B, N=N, H=8, d=d, De=De, dtype=L.EGT_BF16 if bf else L.EGT_F32, flags=flags, clip_lo=-5.0,
                           clip_hi=5.0, random_mask_prob=0.1, ln_eps=1e-5, reserved=0, seed=0, seed_device=None)
        p = C.byref(desc)
        if not egt_lib.egt_block_supported(p):
            continue
        n += 1
        assert egt_lib.egt_block_saved_bytes(p) == egt_lib.egt_stack_saved_bytes(p, 1) > 0, name
        assert egt_lib.egt_block_workspace_bytes(p) == egt_lib.egt_stack_workspace_bytes(p, 1) > 0, name
    assert n == len(cases())   # every plan case is a supported descriptor


# --------------------------------------------------------------------------------------------------- argument errors ---
PTR = 0x1000   # a non-NULL dummy: every call below is answered before anything is dereferenced or launched


def _desc(L, De=64, flags=0, prob=0.0):
    return L.BlockDesc(B=2, N=19, H=8, d=8, De=De, dtype=L.EGT_F32, flags=L.BF_GATE | L.BF_CLIP | flags, clip_lo=-5.0,
                       clip_hi=5.0, random_mask_prob=prob, ln_eps=1e-3, reserved=0, seed=7, seed_device=None)


def _tables(L, layers):
    t = (L.BlockParams * layers)()
    for s in t:
        for f in L.BLOCK_PARAM_FIELDS:
            setattr(s, f, PTR)
    return t


def _call(lib, L, entry, desc, layers=3, params="ok", grads="ok", h=PTR, attn_mask=None, rand_mask=None, alias=False):
    """one call of `entry` with dummy pointers everywhere except where the case says otherwise"""
    stack = entry.startswith("egt_stack")
    n = max(layers, 1) if stack else 1
    p = _tables(L, n) if params == "ok" else params
    g = _tables(L, n) if grads == "ok" else grads
    lay = (layers,) if stack else ()
    rm = () if stack else (rand_mask,)
    if entry.endswith("fwd"):      # desc [layers] params h e key_mask attn_mask [rand_mask] h_out e_out saved ws stream
        args = (C.byref(desc), *lay, p, h, PTR, None, attn_mask, *rm, PTR, PTR, PTR, PTR, None)
    else:                          # ... saved d_h_out d_e_out d_h d_e grads ws stream
        d_h_out = PTR + 64
        args = (C.byref(desc), *lay, p, h, PTR, None, attn_mask, *rm, PTR, d_h_out, PTR, d_h_out if alias else PTR, PTR, g, PTR, None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.egt_last_error_string().decode()


ENTRIES = ("egt_block_fwd", "egt_block_bwd", "egt_stack_fwd", "egt_stack_bwd")


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors(egt_lib, entry):
    from egt_amd import _lib as L
    lib = egt_lib
    stack, bwd = entry.startswith("egt_stack"), entry.endswith("bwd")

    def expect(code, text, **kw):
        desc = kw.pop("desc", None) or _desc(L)
        rc, msg = _call(lib, L, entry, desc, **kw)
        assert rc == code and text in msg, (entry, kw, rc, msg)

    expect(L.EGT_E_NULL, "params/" if stack else "params is NULL", params=None)
    expect(L.EGT_E_NULL, "h/e/saved/d_h_out/d_e_out/d_h/d_e/" if bwd else "h/e/h_out/e_out/saved/workspace is NULL", h=None)
    expect(L.EGT_E_NULL, "ATTN_MASK set but attn_mask is NULL", desc=_desc(L, flags=L.BF_ATTN_MASK))
    if bwd:
        expect(L.EGT_E_FLAGS, "d_h must not alias d_h_out", alias=True)
    static = L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN
    if stack:
        expect(L.EGT_E_SHAPE, "layers must be >= 1", layers=0)
        expect(L.EGT_E_SHAPE, "at most 64 layers per stack call", layers=65)
        expect(L.EGT_E_FLAGS, "egt_stack_* does not take EGT_BF_STATIC_EDGE", desc=_desc(L, De=8, flags=static))
        expect(L.EGT_E_FLAGS, "egt_stack_* does not take EGT_BF_STATIC_EDGE", desc=_desc(L, De=8, flags=static), h=None)   # flags before pointers
    else:
        expect(L.EGT_E_FLAGS, "takes the in-kernel random mask only", desc=_desc(L, De=8, flags=static | L.BF_TRAINING, prob=0.1),
               rand_mask=PTR)
    if bwd:
        g = _tables(L, 3 if stack else 1)
        g[2 if stack else 0].dense_qkv_kernel = None
        expect(L.EGT_E_NULL, "layer 2 gradient pointer #8 is NULL" if stack else "gradient pointer #8 is NULL", grads=g)
        if stack:   # the direction's first layer with a NULL slot is the one reported: the backward starts at the top
            g[0].norm_mha_gamma = None
            expect(L.EGT_E_NULL, "layer 2 gradient pointer #8 is NULL", grads=g)
    p = _tables(L, 3 if stack else 1)
    p[2 if stack else 0].dense_mha_bias = None
    expect(L.EGT_E_NULL, "block parameter #11 is NULL", params=p)


# ------------------------------------------------------------------------------------------------------- route table ---
def _case(name, want, N=19, edge="f32", attn_mask=False, rand_mask=False, train=False, in_stack=False, no_static=False, **kw):
    kw = dict(dict(num_heads=8, model_width=64, edge_width=64), **kw)
    return dict(name=name, want=want, N=N, edge=edge, attn_mask=attn_mask, rand_mask=rand_mask, train=train, in_stack=in_stack,
                no_static=no_static, kw=kw)


RES, BIAS = ("fused", "chained-residual"), ("fused", "per-layer-bias")
COMPOSED = ("composed", None)
NARROW = dict(model_width=64, edge_width=8)
ROUTE_CASES = [
    _case("config1_d8_De64", RES),
    _case("config2_d6_De48", RES, model_width=48, edge_width=48),
    _case("config3_d8_De8_bf16", RES, edge="bf16", **NARROW),
    _case("config4_d8_De8", RES, **NARROW),
    _case("config5_d64_De32", ("fused-pair", None), N=16, model_width=512, edge_width=32),
    _case("constrained_mask", RES, attn_mask=True, edge_channel_type="constrained"),
    _case("constrained_no_mask", COMPOSED, edge_channel_type="constrained"),
    _case("bias_alone", BIAS, edge_channel_type="bias", **NARROW),
    _case("bias_in_stack", ("fused", "static"), in_stack=True, edge_channel_type="bias", **NARROW),
    _case("bias_in_stack_De64", BIAS, in_stack=True, edge_channel_type="bias"),
    _case("bias_in_stack_no_static_edge", BIAS, in_stack=True, no_static=True, edge_channel_type="bias", **NARROW),
    _case("none", COMPOSED, edge_channel_type="none"),
    _case("add_n_norm", COMPOSED, add_n_norm=True),
    _case("node_dropout_train", COMPOSED, train=True, node_dropout=0.1),
    _case("node_dropout_eval", RES, node_dropout=0.1),
    _case("attn_dropout", COMPOSED, attn_dropout=0.1),
    _case("virtual_node", COMPOSED, num_virtual_nodes=1),
    _case("fused_off", COMPOSED, fused="off"),
    _case("fused_true_uncoverable", RuntimeError, add_n_norm=True, fused=True),
    _case("host_rand_mask", RES, rand_mask=True, train=True, random_mask_prob=0.1),
    _case("host_rand_mask_bias_in_stack", BIAS, rand_mask=True, train=True, in_stack=True, random_mask_prob=0.1,
          edge_channel_type="bias", **NARROW),
    _case("bf16_d64", COMPOSED, N=16, edge="bf16", model_width=512, edge_width=32),
]
EDGE_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}


def make_block(case):
    """the block of a route case, opted into the static-edge route the way EGTLayerStack does it"""
    from egt_amd.layers import EGTBlock
    blk = EGTBlock(**case["kw"])
    blk.train(case["train"])
    if case["in_stack"]:
        blk._static_edge, blk._static_first = True, True
    return blk


@pytest.fixture
def static_edge_switch():
    """EGT_NO_STATIC_EDGE is read once per process: set the remembered answer for a case, restore it afterwards"""
    from egt_amd import fused as FZ
    old = FZ._NO_STATIC_EDGE

    def set_(off):
        FZ._NO_STATIC_EDGE = bool(off)
    yield set_
    FZ._NO_STATIC_EDGE = old


@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: c["name"])
def test_route_table(egt_lib, static_edge_switch, case):
    from egt_amd import fused as FZ
    blk = make_block(case)
    static_edge_switch(case["no_static"])
    args = (blk, 2, case["N"], torch.float32, EDGE_DTYPE[case["edge"]], True)
    kw = dict(attn_mask=case["attn_mask"], rand_mask=case["rand_mask"], training=case["train"])
    if case["want"] is RuntimeError:
        with pytest.raises(RuntimeError, match="not covered"):
            FZ.route_core(*args, **kw)
        return
    assert FZ.route_core(*args, **kw) == case["want"]
    assert FZ.route_core(*args[:5], False, **kw) == COMPOSED          # not on the GPU: nothing fused
    if case["want"][0] == "fused-pair":                                # injected dropout samples keep the pair operator out
        assert FZ.route_core(*args, keep=True, **kw) == COMPOSED


def test_bf16_refusal_messages(egt_lib):
    from egt_amd import fused as FZ
    by_name = {c["name"]: c for c in ROUTE_CASES}
    why = FZ.bf16_refusal(make_block(by_name["bf16_d64"]))
    assert why is not None and "head dim 64" in why and "not covered by the fused block" in why
    assert FZ.bf16_refusal(make_block(by_name["config3_d8_De8_bf16"])) is None
    assert FZ.bf16_refusal(make_block(by_name["bias_in_stack"])) is None
    assert FZ.bf16_refusal(make_block(by_name["fused_off"])) == "the fused block is switched off"
    assert FZ.bf16_refusal(make_block(by_name["add_n_norm"])) == "add_n_norm / edge_activation"
    assert FZ.bf16_refusal(make_block(by_name["node_dropout_eval"])) == "node / edge dropout"   # a model trains
    assert FZ.bf16_refusal(make_block(by_name["none"])) == "edge_channel_type 'none'"


def test_memo_follows_the_block(egt_lib, static_edge_switch):
    """the memo's key is built from the block's attributes as they are: flipping one between calls cannot return a stale answer"""
    from egt_amd import fused as FZ
    static_edge_switch(False)
    blk = make_block({c["name"]: c for c in ROUTE_CASES}["bias_in_stack"])
    args = (blk, 2, 19, torch.float32, torch.float32, True)
    assert FZ.route_core(*args) == ("fused", "static")
    blk._static_edge = False
    assert FZ.route_core(*args) == BIAS
    blk._static_edge = True
    assert FZ.route_core(*args) == ("fused", "static")
    blk.edge_width = 64                       # another descriptor: another answer (the static route is a De = 8 one)
    assert FZ.route_core(*args) == BIAS
    blk.edge_width = 8
    assert FZ.route_core(*args) == ("fused", "static")
    n = len(FZ._LIB_ANSWERS)
    FZ.route_core(*args)
    assert len(FZ._LIB_ANSWERS) == n          # answered from the memo
