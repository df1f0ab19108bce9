"""The HIP kernels against what the REFERENCE'S OWN code computed (tests/golden/reference/, written by
tests/golden/make_reference_golden.py from the reference's model code run unmodified on the eager stand-in).  Reads the
fixtures only, never the reference tree.

Every block-level case on the composed path and on every fused route that covers it (fused block, one-call stack, MFMA inner
op at d = 16 / 64, the De = 8 kernels, the FFN at widths 64 / 48 / 16); every model-level case as one forward and backward of
the product model.  Tolerances are util.FWD / util.BWD; masks and the distance target are bit-exact.

The fixtures hold, per tensor, the whole tensor up to a cap (512 elements at block level, 128 for stacks and models) or that
many sampled elements, and sum, sum of squares and max |x| of the whole tensor (tests/reference_cases.py).  `close` holds the
stored elements to both halves of the tolerance (element-wise, normalised L2) and the WHOLE tensor to the stored sums.
Inputs and weights come from the seeded recipes and are checked against the digests the fixture stores.  Every fused test
asserts the route that ran."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases as CS
import reference_cases as RC
import virtual_nodes_ref as VR
from test_block_gpu import FUSED_CASES, PMAP, build_block
from util import assert_close, FWD, BWD

pytestmark = pytest.mark.gpu

FWD_KEYS = {"V_att", "H_hat", "A_tild", "h_out", "e_out", "y", "loss", "distance_loss"}


def check_digests(fix, inputs, weights):
    for grp, d in (("inputs", inputs), ("weights", weights)):
        for k, v in d.items():
            if v is not None:
                assert np.array_equal(RC.sha(v), fix["sha"][f"{grp}/{k}"]), f"{grp}/{k}: the recipe no longer gives the fixture's array"


def close(fix, key, actual):
    """`actual` (the WHOLE tensor of the code under test) against the fixture's record of `key`:
      * the stored elements under util.FWD / util.BWD: the element-wise term with the absolute part relative to the whole
        tensor's max |x| (`floor`), and the normalised L2 bound over the stored elements, always;
      * sum and sum of squares of the whole tensor against the stored ones, at the bounds the same tolerances imply: every
        element may be off by arel * max + rtol * |r_i|, so |sum a - sum r| <= n * arel * max + rtol * sqrt(n * sum r^2)
        (Cauchy-Schwarz for sum |r_i|); ||a - r|| <= l2 * ||r|| gives | ||a||^2 - ||r||^2 | <= l2 * (2 + l2) * ||r||^2.
    A tensor that is identically zero in exact arithmetic (max |r| < 1e-9, as in tests/util.py) is held to zero_atol."""
    tol = dict(FWD if key in FWD_KEYS else BWD)
    l2, zero_atol = tol.pop("l2"), BWD["zero_atol"]
    s, ss, mx = (float(v) for v in fix["stat"][key])
    a, r = RC.picked(fix, key, actual), torch.from_numpy(fix[f"out/{key}"]).double()
    whole = actual.detach().double().cpu().reshape(-1)
    assert torch.isfinite(whole).all(), f"{key}: non-finite values"
    n = max(whole.numel(), 1)
    if mx < 1e-9:
        assert float(whole.abs().max()) <= zero_atol, f"{key}: analytically zero, |value| up to {float(whole.abs().max()):.3e}"
        return
    assert_close(a, r, name=key, floor=mx, **{k: v for k, v in tol.items() if k != "zero_atol"})
    rel = float((a - r).norm()) / float(r.norm())
    assert rel <= l2, f"{key}: normalised L2 error {rel:.3e} > {l2:.1e} over the stored elements"
    ds, bs = abs(float(whole.sum()) - s), n * tol["arel"] * mx + tol["rtol"] * (n * ss) ** 0.5
    assert ds <= bs, f"{key}: sum of the whole tensor off by {ds:.3e} > {bs:.3e}"
    dq, bq = abs(float((whole * whole).sum()) - ss), l2 * (2 + l2) * ss
    assert dq <= bq, f"{key}: sum of squares of the whole tensor off by {dq:.3e} > {bq:.3e}"


def close_or_zero(fix, key, grad):
    """a gradient against the fixture; where the reference's is identically zero (a weight off every path to the loss) the
    product's is absent or zero"""
    if float(fix["stat"][key][2]) == 0.0:
        assert grad is None or float(grad.abs().max()) == 0.0, f"{key}: the reference's gradient is identically zero"
        return
    assert grad is not None, f"{key}: no gradient"
    close(fix, key, grad)


# --------------------------------------------------------------------------------------------------- inner op -----
@pytest.mark.parametrize("name", RC.ATTN_NAMES)
def test_inner_op(name, gpu, egt_lib):
    from test_attn_gpu import run_hip
    fix = RC.load("attn", name)
    inp, attrs, _ = RC.make_attn_case(name)
    check_digests(fix, inp, {})
    out = run_hip(inp, attrs, gpu)
    for k in ("V_att", "H_hat", "A_tild", "dQKV", "dE", "dG"):
        if f"out/{k}" in fix:
            close(fix, k, out[k])


@pytest.mark.parametrize("name,d", [("mfma_d16_n37", 16), ("d64", 64)])
def test_inner_op_mfma(name, d, gpu, egt_lib):
    """the MFMA-tiled inner op (eight heads, d in {16, 32, 64}; taken when A_tild is not asked for)"""
    import ctypes as C
    from egt_amd import _lib, AttnConfig
    from egt_amd.functional import _attn_desc
    from test_attn_gpu import run_hip
    fix = RC.load("attn", name)
    inp, attrs, c = RC.make_attn_case(name)
    assert c["d"] == d
    cfg = AttnConfig(num_heads=attrs["num_heads"], clip_logits_value=attrs["clip_logits_value"], need_a_tild=False)
    desc = _attn_desc(cfg, c["B"], c["N"], d, True, True, False)
    assert _lib.load().egt_attn_mfma_supported(C.byref(desc), 0), "the MFMA kernels do not cover this case"
    out = run_hip(inp, attrs, gpu, a_tild=False)
    for k in ("V_att", "H_hat", "dQKV", "dE", "dG"):
        close(fix, k, out[k])


# ------------------------------------------------------------------------------------------------------ block -----
def _compare_block(fix, out, dparams):
    for k in ("h_out", "e_out", "dh", "de"):
        close(fix, k, out[k])
    for k in fix["stat"]:
        if k.startswith("d/"):
            close_or_zero(fix, k, dparams.get(k[2:]))


@pytest.mark.parametrize("name", list(CS.BLOCK_CASES))
def test_block_composed(name, gpu, egt_lib):
    from test_block_gpu import run_block
    fix = RC.load("block", name)
    out, dparams, (inp, params, _) = run_block(name, gpu, fused=False)
    check_digests(fix, inp, params)
    _compare_block(fix, out, dparams)


def _run_fused(name, gpu):
    """test_block_gpu.run_block(name, fused=True), keeping the block so that the route it took can be asserted"""
    inp, params, attrs, c = CS.make_block_case(name)
    blk = build_block(c, attrs, params, gpu, True)
    blk.train(c.get("rand_p") is not None)
    cu = lambda t: None if t is None else t.to(gpu)
    h = cu(inp["h"]).requires_grad_(); e = cu(inp["e"]).requires_grad_()
    h2, e2 = blk(h, e, cu(inp["mask"]), cu(inp["attn_mask"]), rand_mask=cu(inp["rand_mask"]))
    ((h2 * cu(inp["dh"])).sum() + (e2 * cu(inp["de"])).sum()).backward()
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad)
    return blk, out, {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items() if hasattr(blk, m)}, (inp, c)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_block_fused(name, gpu, egt_lib):
    """the fused block, route asserted; residual_pattern (De = 8) must reach the De = 8 kernels"""
    import ctypes as C
    from egt_amd import fused as FZ
    blk, out, dparams, (inp, c) = _run_fused(name, gpu)
    assert blk.last_path in ("fused", "fused-pair"), blk.last_path
    if c["De"] == 8:
        form = egt_lib.egt_block_launch_form(C.byref(FZ._desc(blk, c["B"], c["N"], blk.training, 0)))
        assert form is not None and b"fwd=k_narrow_fwd" in form and b"bwd=k_narrow_bwd" in form, form
    _compare_block(RC.load("block", name), out, dparams)


@pytest.mark.parametrize("name", ["residual_zinc500k", "residual_zinc100k", "residual_pattern", "residual_n64", "ungated_residual", "bias"])
def test_block_through_the_stack_call(name, gpu, egt_lib):
    """the same cases as a one-layer EGTStack: one C call per direction"""
    from egt_amd import EGTStack
    fix = RC.load("block", name)
    inp, params, attrs, c = CS.make_block_case(name)
    st = EGTStack(model_height=1, model_width=c["Dh"], edge_width=c["De"], num_heads=8, gate_attention=attrs["gate_attention"],
                  edge_channel_type=attrs["edge_channel_type"], random_mask_prob=0.0, fused=True).to(gpu).eval()
    blk = st.blocks[0]
    with torch.no_grad():
        for k, (m, a) in PMAP.items():
            if hasattr(blk, m):
                getattr(getattr(blk, m), a).copy_(params[k].to(gpu))
    h = inp["h"].to(gpu).requires_grad_(); e = inp["e"].to(gpu).requires_grad_()
    h2, e2 = st(h, e, inp["mask"].to(gpu))
    assert st.last_path == "fused-stack"
    torch.autograd.backward([h2, e2], [inp["dh"].to(gpu), inp["de"].to(gpu)])
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad)
    _compare_block(fix, out, {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items() if hasattr(blk, m)})


# (edge_channel_type 'none' has no edge channels: mha_block alone, nothing to route and nothing reported -- tests/test_route_gpu.py)
@pytest.mark.parametrize("name,route", [(n, r) for n, v in RC.BLOCK_VARIANTS.items() for r in ("composed", "fused")
                                        if not (v.get("ect") == "none" and r == "fused")])
def test_block_variants(name, route, gpu, egt_lib):
    """add_n_norm and node / edge dropout with the injected keep masks, built as tests/test_block_variants_gpu.py builds them:
    on the composed path, and on the fused block wherever it covers the variant (where it does not, it must say so)"""
    from egt_amd import EGTBlock
    fix = RC.load("block", name)
    inp, params, attrs = RC.block_inputs(name)
    check_digests(fix, inp, params)
    Dh, De = inp["h"].shape[-1], inp["e"].shape[-1]
    drop = "node_dropout" in attrs
    kw = dict(node_dropout=attrs["node_dropout"], edge_dropout=attrs["edge_dropout"]) if drop else \
        dict(gate_attention=attrs["gate_attention"], edge_channel_type=attrs["edge_channel_type"], add_n_norm=True)
    blk = EGTBlock(model_width=Dh, edge_width=De, num_heads=8, fused=route == "fused", **kw).to(gpu).train(drop)
    with torch.no_grad():
        for k, (m, a) in PMAP.items():
            if hasattr(blk, m):
                getattr(getattr(blk, m), a).copy_(params[k].to(gpu))
    h = inp["h"].to(gpu).requires_grad_(); e = inp["e"].to(gpu).requires_grad_()
    fkw = dict(node_keep=inp["node_keep"].to(gpu), edge_keep=inp["edge_keep"].to(gpu)) if drop else {}
    try:
        h2, e2 = blk(h, e, inp["mask"].to(gpu), **fkw)
    except RuntimeError as ex:
        assert route == "fused" and "not covered" in str(ex), ex
        return
    if attrs["edge_channel_type"] == "none":
        assert not hasattr(blk, "last_path")
    else:
        assert blk.last_path == "composed" if route == "composed" else blk.last_path in ("fused", "fused-pair"), blk.last_path
    torch.autograd.backward([h2, e2], [inp["dh"].to(gpu), inp["de"].to(gpu)])
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad if e.grad is not None else torch.zeros_like(e))
    _compare_block(fix, out, {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items() if hasattr(blk, m)})


# -------------------------------------------------------------------------------------------------------- FFN -----
@pytest.mark.parametrize("name", list(CS.FFN_CASES))
def test_ffn(name, gpu, egt_lib):
    from egt_amd import ffn
    fix = RC.load("ffn", name)
    inp, params, c = CS.make_ffn_case(name)
    check_digests(fix, inp, params)
    prm = {k: params[k].to(gpu).requires_grad_() for k in CS.FFN_NAMES}
    x = inp["x"].to(gpu).requires_grad_()
    y = ffn(x, *[prm[k] for k in CS.FFN_NAMES], activation=c["act"])
    y.backward(inp["dy"].to(gpu))
    close(fix, "y", y)
    close(fix, "dx", x.grad)
    for k in CS.FFN_NAMES:
        close(fix, f"d/{k}", prm[k].grad)


# ------------------------------------------------------------------------------------------------------ stack -----
@pytest.mark.parametrize("name", list(RC.STACK_CASES))
def test_two_layer_stack_with_ffns_and_final_norms(name, gpu, egt_lib):
    from egt_amd import EGTLayerStack, KerasLayerNorm
    fix = RC.load("stack", name)
    inp, params, cfg = RC.stack_inputs(name)
    check_digests(fix, inp, params)
    st = EGTLayerStack(model_height=cfg["model_height"], model_width=cfg["model_width"], edge_width=cfg["edge_width"],
                       num_heads=8, fused=True).to(gpu).eval()
    model = SimpleNamespace(layers=st, node_norm_final=KerasLayerNorm(cfg["model_width"]).to(gpu),
                            edge_norm_final=KerasLayerNorm(cfg["edge_width"]).to(gpu))
    with torch.no_grad():
        for k, v in params.items():
            VR.module_param(model, k).copy_(v.to(gpu))
    h = inp["h"].to(gpu).requires_grad_(); e = inp["e"].to(gpu).requires_grad_()
    h2, e2 = st(h, e, inp["mask"].to(gpu))
    assert [b.last_path for b in st.blocks] == ["fused"] * cfg["model_height"] and st.last_edge_route != "composed"
    if cfg["edge_width"] == 8:
        import ctypes as C
        from egt_amd import fused as FZ
        form = egt_lib.egt_block_launch_form(C.byref(FZ._desc(st.blocks[0], h.shape[0], h.shape[1], False, 0)))
        assert form is not None and b"fwd=k_narrow_fwd" in form and b"bwd=k_narrow_bwd" in form, form
    h2, e2 = model.node_norm_final(h2), model.edge_norm_final(e2)
    torch.autograd.backward([h2, e2], [inp["dh"].to(gpu), inp["de"].to(gpu)])
    for k, v in dict(h_out=h2, e_out=e2, dh=h.grad, de=e.grad).items():
        close(fix, k, v)
    for k in params:
        close(fix, f"d/{k}", VR.module_param(model, k).grad)


# ----------------------------------------------------------------------------------------------------- models -----
HEAD_KEYS = ("edge_norm_final.", "mlp_out_dist_targ_", "distance_target.")


def _build_model(name, gpu):
    from egt_amd import ZincDCTransformer, Cifar10DCTransformer
    kind, inp, params, cfg, v = RC.model_inputs(name)
    if kind == "cifar10":
        model = Cifar10DCTransformer(model_width=cfg["model_width"], edge_width=cfg["edge_width"], model_height=cfg["model_height"],
                                     upto_hop=cfg["upto_hop"], random_mask_prob=0.0)
    else:
        model = ZincDCTransformer(random_mask_prob=0.0, **{**cfg, **v})
    return kind, inp, params, cfg, v, model.to(gpu).eval()


def _param(model, named, key):
    if key.startswith(HEAD_KEYS):
        return named.get(key.replace(".", "/"))
    return VR.module_param(model, key)


def test_distance_objective_is_refused_at_width_16(gpu, egt_lib):
    """zinc_small_dist: the reference's numbers are in the fixture (and pin the oracle on the CPU); the product builds the
    fused distance head for model widths 48 and 64 and says so"""
    with pytest.raises(NotImplementedError, match="distance_loss"):
        _build_model("zinc_small_dist", gpu)


@pytest.mark.parametrize("name", [n for n in RC.MODEL_NAMES if n != "zinc_small_dist"])
def test_model_forward_backward(name, gpu, egt_lib):
    from egt_amd import mae_loss, sparse_xent_loss
    fix = RC.load("model", name)
    kind, inp, params, cfg, v, model = _build_model(name, gpu)
    check_digests(fix, inp, params)
    named = model.keras_named_parameters()
    loaded = set()
    with torch.no_grad():
        for k, t in params.items():
            prm = _param(model, named, k)
            if prm is not None:
                prm.copy_(t.to(gpu)); loaded.add(id(prm))
    assert {id(p) for p in named.values()} <= loaded, "a named parameter of the model that the fixture does not hold"
    dev = lambda k: inp[k].to(gpu)
    y, aux = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"), return_aux=True)
    loss = sparse_xent_loss(y, dev("target")) if kind == "cifar10" else mae_loss(y, dev("target"))
    if "distance_loss" in v:
        close(fix, "distance_loss", aux["distance_loss"])
        loss = loss + v["distance_loss"] * aux["distance_loss"].mean()
    loss.backward()
    close(fix, "y", y)
    close(fix, "loss", loss.reshape(1))
    # what the model produces on the way: bit-exact
    nv = v.get("num_virtual_nodes", 0)
    _, _, mask = model.embeddings(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
    assert np.array_equal(RC.sha(mask.to(torch.bool).cpu()), fix["sha"]["bits/node_mask"]), "node mask"
    if cfg.get("edge_channel_type") == "constrained":
        M = model.edge_mask(dev("graph_matrix"), None)
        assert np.array_equal(RC.sha(M.to(torch.uint8).cpu()), fix["sha"]["bits/edge_mask"]), "edge mask"
    if "distance_loss" in v:
        from egt_amd.head import distance_target
        tgt = distance_target(dev("graph_matrix"), v["distance_target"])
        assert np.array_equal(RC.sha(tgt.to(torch.int64).cpu()), fix["sha"]["bits/distance_target"]), "distance target"
    assert {k for k in fix["sha"] if k.startswith("bits/")} == \
        {"bits/node_mask"} | ({"bits/edge_mask"} if cfg.get("edge_channel_type") == "constrained" else set()) | \
        ({"bits/distance_target"} if "distance_loss" in v else set())
    live = {id(p) for p in named.values()}
    checked = 0
    for k in params:
        prm = _param(model, named, k)
        if prm is None or id(prm) not in live:     # not a parameter of the Keras model: the reference's gradient is zero
            assert float(fix["stat"][f"d/{k}"][2]) == 0.0, f"{k}: the reference trains it, the model does not own it"
            assert prm is None or prm.grad is None or float(prm.grad.abs().max()) == 0.0, k
            continue
        close_or_zero(fix, f"d/{k}", prm.grad); checked += 1
    assert checked == len(named)
