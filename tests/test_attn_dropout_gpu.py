"""Attention dropout on the fused block (EGT_BF_ATTN_DROPOUT, EGTBlock(fused_attn_dropout=True)): forward, backward and the fourteen
parameter gradients of the DO instances of the MFMA-tile pair kernels against the fp64 oracle (oracle.egt_oracle.block_forward with
drop_keep / attn_dropout), which is fed rng_ref.dropout_keep -- and rng_ref.random_mask where the recipe sets a random mask -- of the
seed the block consumed.  Tolerances: the suite's FWD / BWD, compared as tests/test_block_gpu.py compares them; bf16 rows under the
single-operator bf16 contract of tests/test_bf16_edges_gpu.py (the oracle reads the same bf16 inputs; bf16_stack_tol(1)).  Which
kernels a shape reaches is asserted through egt_block_launch_form / egt_block_bwd_kernel, so a plan change cannot hide a family.

EGT_ATTN_DROPOUT_MARGINS=<path>: the worst error / tolerance of every parity case is written there (JSON) when the module ends."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import attn_dropout_cases as AC
import cases as CS
from test_block_gpu import PMAP
from util import assert_close, margin, bf16_stack_tol, FWD, BWD

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = "tests/" + os.path.basename(__file__)
MARGINS = {}
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    path = os.environ.get("EGT_ATTN_DROPOUT_MARGINS")
    if path and MARGINS:
        old = {}
        if os.path.exists(path):      # (the child runs of this module add their cases to the parent's file)
            try:
                old = json.load(open(path))
            except ValueError:
                old = {}
        old.update(MARGINS)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def build(c, attrs, params, dev, rate, p=0.0, opt_in=True, fused="auto", seed=0):
    from egt_amd import EGTBlock
    blk = EGTBlock(model_width=c["Dh"], edge_width=c["De"], num_heads=8, gate_attention=attrs["gate_attention"],
                   edge_channel_type=attrs["edge_channel_type"], attn_dropout=rate, random_mask_prob=p, fused=fused, seed=seed,
                   fused_attn_dropout=opt_in).to(dev)
    with torch.no_grad():
        for k, (m, a) in PMAP.items():
            if hasattr(blk, m):
                getattr(getattr(blk, m), a).copy_(params[k].to(dev))
    return blk


def run(blk, inp, dev, rand_mask=None, bf16=False):
    cu = lambda t: None if t is None else t.to(dev)
    h = cu(inp["h"]).requires_grad_()
    e = cu(inp["e"].to(BF) if bf16 else inp["e"]).requires_grad_()
    de = cu(inp["de"].to(BF) if bf16 else inp["de"])
    h2, e2 = blk(h, e, cu(inp["mask"]), cu(inp["attn_mask"]), rand_mask=cu(rand_mask))
    torch.autograd.backward([h2, e2], [cu(inp["dh"]), de])
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad)
    dparams = {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items() if hasattr(blk, m)}
    return out, dparams


def run_composed(blk, inp, dev, keep, rand_mask):
    """the composed block (fused='off') given the same samples: EGT.forward's drop_keep is reached through the inner module"""
    cu = lambda t: None if t is None else t.to(dev)
    h = cu(inp["h"]).requires_grad_(); e = cu(inp["e"]).requires_grad_()
    inner = blk.mha.forward
    blk.mha.forward = lambda inputs, mask=None, training=None, rand_mask=None, drop_keep=None: inner(
        inputs, mask=mask, training=training, rand_mask=cu(rand_mask), drop_keep=cu(keep))
    try:
        h2, e2 = blk(h, e, cu(inp["mask"]), cu(inp["attn_mask"]))
    finally:
        del blk.mha.forward
    ((h2 * cu(inp["dh"])).sum() + (e2 * cu(inp["de"])).sum()).backward()
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad)
    dparams = {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items() if hasattr(blk, m)}
    return out, dparams


def compare(tag, out, dparams, ref, bias=False, fwd=FWD, bwd=BWD, pbwd=None):
    ref = dict(ref)
    rd = ref.pop("dparams")
    pbwd = pbwd or bwd
    strip = lambda t: {k: v for k, v in t.items() if k in ("rtol", "arel")}
    m = {}
    for k, tol in (("h_out", fwd), ("e_out", fwd), ("dh", bwd), ("de", bwd)):
        if bias and k == "e_out":
            continue
        m[k] = margin(out[k].float(), ref[k], **strip(tol))
    for k, g in rd.items():
        if g is not None and float(g.abs().max()) >= 1e-9:
            m[k] = margin(dparams[k], g, **strip(pbwd))
    MARGINS[tag] = dict(worst=max(m.values()), by_tensor=m)
    print(f"[attn_dropout margins] {tag}: worst {max(m, key=m.get)} {max(m.values()):.3f}")
    assert_close(out["h_out"], ref["h_out"], name="h_out", **fwd)
    if not bias:
        assert_close(out["e_out"].float(), ref["e_out"], name="e_out", **fwd)
    assert_close(out["dh"], ref["dh"], name="dh", **bwd)
    assert_close(out["de"].float(), ref["de"], name="de", **bwd)
    for k, g in rd.items():
        if g is None:
            assert dparams.get(k) is None or float(dparams[k].abs().max()) == 0.0, k
            continue
        assert_close(dparams[k], g, name=k, **pbwd)


def forms(egt_lib, blk, B, N, edge_dtype=torch.float32):
    """launch form and backward family of the flagged training descriptor of `blk`"""
    from egt_amd import fused as FZ
    desc = FZ._desc(blk, B, N, blk.mha.random_mask_prob > 0, 0, edge_dtype, dropout=True)
    assert egt_lib.egt_block_supported(C.byref(desc)) == 1
    return egt_lib.egt_block_launch_form(C.byref(desc)).decode(), egt_lib.egt_block_bwd_kernel(C.byref(desc)).decode()


def consumed_seed(blk):
    """the seed of the block's LAST call (EGT.next_seed's formula at the current call count)"""
    return AC.first_seed(blk.mha.seed, blk.mha._calls)


def check_forms(form, bk, ffwd, fbwd):
    if not (os.environ.get("EGT_BWD_TL") or os.environ.get("EGT_FWD_ROWS")):
        assert f"fwd={ffwd}" in form and f"bwd={fbwd}/" in form and bk == fbwd, (form, bk)
    else:
        assert fbwd in form and bk == fbwd, (form, bk)


ROWS = list(AC.SHAPES) + list(AC.VARIANTS)
_ROW_CACHE = {}


def row_results(row, recipe, gpu, egt_lib):
    """one fused training call of a table row and its oracle, computed once and shared by the tests that read them"""
    key = (row, recipe)
    if key not in _ROW_CACHE:
        rate, prob = AC.RATES[recipe]
        inp, params, attrs, c, ffwd, fbwd = AC.make_row(row)
        blk = build(c, attrs, params, gpu, rate, p=prob).train()
        form, bk = forms(egt_lib, blk, c["B"], c["N"])
        out, dparams = run(blk, inp, gpu)
        assert blk.last_path == "fused", blk.last_path
        assert blk.mha._calls == 1
        seed = consumed_seed(blk)
        keep, rm = AC.keep_of(seed, c["B"], c["N"], rate), AC.rand_of(seed, c["B"], c["N"], prob)
        ref = AC.oracle(inp, params, attrs, rate, keep, rm)
        _ROW_CACHE[key] = dict(inp=inp, params=params, attrs=attrs, c=c, out=out, dparams=dparams, ref=ref, keep=keep, rm=rm,
                               form=form, bk=bk, ffwd=ffwd, fbwd=fbwd, rate=rate, prob=prob)
    return _ROW_CACHE[key]


@pytest.mark.parametrize("recipe", list(AC.RATES))
@pytest.mark.parametrize("row", ROWS)
def test_block_vs_oracle(row, recipe, gpu, egt_lib):
    r = row_results(row, recipe, gpu, egt_lib)
    check_forms(r["form"], r["bk"], r["ffwd"], r["fbwd"])
    compare(f"{row}-{recipe}", r["out"], r["dparams"], r["ref"], bias=r["attrs"]["edge_channel_type"] == "bias")


@pytest.mark.parametrize("recipe", list(AC.RATES))
@pytest.mark.parametrize("row", ROWS)
def test_block_vs_composed(row, recipe, gpu, egt_lib):
    """the same rows against the composed block (egt_attn.hip's drop_factor path) given the same keep tensor: two fp32 routes
    against each other, twice FWD / BWD"""
    r = row_results(row, recipe, gpu, egt_lib)
    blk = build(r["c"], r["attrs"], r["params"], gpu, r["rate"], p=r["prob"], opt_in=False, fused="off").train()
    out, dparams = run_composed(blk, r["inp"], gpu, r["keep"], r["rm"])
    assert blk.last_path == "composed"
    bias = r["attrs"]["edge_channel_type"] == "bias"
    two = lambda t: dict(rtol=2 * t["rtol"], arel=2 * t["arel"])
    for k, tol in (("h_out", FWD), ("e_out", FWD), ("dh", BWD), ("de", BWD)):
        if not (bias and k == "e_out"):
            assert_close(r["out"][k], out[k], name=f"{k} fused vs composed", **two(tol))
    floor = float(dparams["attention_gates.bias"].abs().max()) if "attention_gates.bias" in dparams and dparams["attention_gates.bias"] is not None else 0.0
    for k, g in dparams.items():
        if g is None or r["dparams"].get(k) is None:
            continue
        # d(dense_edge_b.bias) is analytically zero (a shift of a row's logits): rounding noise on both routes
        fl = floor if k == "dense_edge_b.bias" else 0.0
        assert_close(r["dparams"][k], g, name=f"{k} fused vs composed", floor=fl, **two(BWD))


@pytest.mark.parametrize("row", list(AC.BF16_ROWS))
@pytest.mark.parametrize("recipe", list(AC.RATES))
def test_bf16_rows(row, recipe, gpu, egt_lib):
    """bf16 edge tensors: the oracle reads the same bf16-rounded e and de'; single-operator bf16 tolerance"""
    rate, prob = AC.RATES[recipe]
    inp, params, attrs, c, _, _ = AC.make_row(row, "bf16")
    ffwd, fbwd = AC.BF16_ROWS[row]
    blk = build(c, attrs, params, gpu, rate, p=prob).train()
    form, bk = forms(egt_lib, blk, c["B"], c["N"], BF)
    check_forms(form, bk, ffwd, fbwd)
    out, dparams = run(blk, inp, gpu, bf16=True)
    assert blk.last_path == "fused" and out["e_out"].dtype == BF and out["de"].dtype == BF
    seed = consumed_seed(blk)
    inp_r = dict(inp, e=inp["e"].to(BF).float(), de=inp["de"].to(BF).float())
    ref = AC.oracle(inp_r, params, attrs, rate, AC.keep_of(seed, c["B"], c["N"], rate), AC.rand_of(seed, c["B"], c["N"], prob))
    tol, ptol = bf16_stack_tol(1), bf16_stack_tol(1, params=True)
    compare(f"bf16-{row}-{recipe}", out, dparams, ref, fwd=tol, bwd=tol, pbwd=ptol)


@pytest.mark.parametrize("row", ["n19_de64", "n69_de8"])
@pytest.mark.parametrize("prob", [0.3, 0.0])
def test_injected_random_mask_with_in_kernel_dropout(row, prob, gpu, egt_lib):
    """a host random-mask tensor (the ML instances, De = 8 included) while the dropout mask is the kernels' own: the call still consumes
    one seed; with random_mask_prob == 0 the tensor is ignored, as the reference ignores it, and the seed is consumed all the same"""
    B, N, d, De, nodes, _, _ = AC.SHAPES[row]
    inp, params, attrs, c = AC.make_case(B, N, d, De, nodes, row + "rm", rand_p=0.3)
    blk = build(c, attrs, params, gpu, 0.25, p=prob).train()
    out, dparams = run(blk, inp, gpu, rand_mask=inp["rand_mask"])
    assert blk.last_path == "fused" and blk.mha._calls == 1
    keep = AC.keep_of(consumed_seed(blk), B, N, 0.25)
    compare(f"injected-rm-{row}-p{prob}", out, dparams, AC.oracle(inp, params, attrs, 0.25, keep, inp["rand_mask"] if prob > 0 else None))


def test_eval_runs_the_unflagged_kernels(gpu, egt_lib):
    """eval() of an opted-in block: bit for bit a block with attn_dropout = 0, and no seed is consumed"""
    inp, params, attrs, c, _, _ = AC.make_row("n19_de64")
    a = build(c, attrs, params, gpu, 0.25, p=0.1).eval()
    b = build(c, attrs, params, gpu, 0.0, p=0.1, opt_in=False).eval()
    oa, ga = run(a, inp, gpu)
    ob, gb = run(b, inp, gpu)
    assert a.last_path == b.last_path == "fused" and a.mha._calls == 0
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_two_calls_draw_different_masks(gpu, egt_lib):
    """each call consumes a fresh seed: the second call's outputs follow the SECOND seed's mask (and differ from the first call's);
    forward and backward of one call share the mask -- the gradients match the oracle of that call's mask"""
    inp, params, attrs, c, _, _ = AC.make_row("n19_de64")
    blk = build(c, attrs, params, gpu, 0.25, seed=5).train()
    o1, _ = run(blk, inp, gpu)
    blk.zero_grad()
    o2, g2 = run(blk, inp, gpu)
    assert blk.mha._calls == 2
    assert not torch.equal(o1["h_out"], o2["h_out"])
    assert torch.equal(o1["e_out"], o2["e_out"])                    # e' does not see the mask
    k1, k2 = (AC.keep_of(AC.first_seed(5, n), c["B"], c["N"], 0.25) for n in (1, 2))
    assert not torch.equal(k1, k2)
    compare("second-call", o2, g2, AC.oracle(inp, params, attrs, 0.25, k2))
    wrong = AC.oracle(inp, params, attrs, 0.25, k1)
    assert margin(o2["h_out"], wrong["h_out"], rtol=FWD["rtol"], arel=FWD["arel"]) > 10.0      # (the test can tell the masks apart)
    assert margin(o2["dh"], wrong["dh"], rtol=BWD["rtol"], arel=BWD["arel"]) > 10.0


def test_without_the_opt_in_the_block_stays_composed(gpu, egt_lib):
    inp, params, attrs, c, _, _ = AC.make_row("n16_de64")
    blk = build(c, attrs, params, gpu, 0.25, opt_in=False).train()
    run(blk, inp, gpu)
    assert blk.last_path == "composed"


def test_device_seeds_draw_the_host_sequence(gpu, egt_lib):
    """under DeviceSeeds (what use_hipgraph attaches) the flagged block reads the device word: after one advance it holds what
    next_seed() would have returned, and the outputs equal the eager call's bit for bit"""
    from egt_amd.graph import DeviceSeeds
    inp, params, attrs, c, _, _ = AC.make_row("n19_de64")
    eager = build(c, attrs, params, gpu, 0.1, p=0.1, seed=9).train()
    oe, ge = run(eager, inp, gpu)
    dev = build(c, attrs, params, gpu, 0.1, p=0.1, seed=9).train()
    seeds = DeviceSeeds([dev.mha], gpu)
    seeds.advance()
    od, gd = run(dev, inp, gpu)
    assert dev.last_path == "fused" and dev.mha._calls == 0
    assert seeds.values()[0] == AC.first_seed(9, 1)
    for k in oe:
        assert torch.equal(oe[k], od[k]), k
    for k in ge:
        assert torch.equal(ge[k], gd[k]), k
    seeds.detach()


# ---------------------------------------------------------------------------------------- launch-plane overrides -----
def _child(env, select):
    e = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", HERE, "-k", select],
                       cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


@pytest.mark.skipif(bool(os.environ.get("EGT_DO_CHILD")), reason="a child run does not start children")
@pytest.mark.parametrize("env,select", [({"EGT_BWD_TL": "4"}, "test_block_vs_oracle and n69_de64-p25"),
                                        ({"EGT_FWD_ROWS": "8"}, "test_block_vs_oracle and n37_d6_de48-p10_rm10"),
                                        ({"EGT_BWD_MATMUL": "bf16x3", "EGT_TEST_ZERO_ATOL": "2e-4"}, "test_block_vs_oracle and n19_de64-p25 and not constrained and not ungated and not bias")],
                         ids=["bwd_tl4", "fwd_rows8", "bwd_bf16x3"])
def test_child_process_switches(env, select, gpu):
    """EGT_BWD_TL / EGT_FWD_ROWS / EGT_BWD_MATMUL are read once per process: one parity row each again in a child (bf16x3: v5's
    split-product form, with the zero-sum absolute term tests/test_bwd_modes_gpu.py runs the block suite under)"""
    _child(dict(env, EGT_DO_CHILD="1"), select)


# --------------------------------------------------------------------------------------------------- model / driver -----
@pytest.mark.parametrize("edge", ["f32", "bf16"])
def test_zinc_model_takes_the_fused_route(edge, gpu, egt_lib):
    """ZincDCTransformer(attn_dropout=0.1, fused_attn_dropout=True) in training mode: every block on the fused route, finite
    prediction and gradients; without the key the same fp32 model composes"""
    from egt_amd.model import ZincDCTransformer
    torch.manual_seed(5)
    kw = dict(model_width=64, edge_width=16, model_height=2, upto_hop=4, attn_dropout=0.1, random_mask_prob=0.1)
    m = ZincDCTransformer(fused_attn_dropout=True, edge_dtype=edge, **kw).to(gpu)
    inp, _, c = CS.make_model_case("zinc_small")
    feed = {k: v.to(gpu) for k, v in inp.items() if k != "target"}
    m.train()
    y = m(**feed)
    y.sum().backward()
    blocks = [b for b in m.modules() if type(b).__name__ == "EGTBlock"]
    assert blocks and all(b.last_path == "fused" for b in blocks)
    assert all(b.mha._calls == 1 for b in blocks)
    assert torch.isfinite(y).all() and all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    m.eval()
    assert torch.isfinite(m(**feed)).all() and all(b.last_path == "fused" and b.mha._calls == 1 for b in blocks)
    if edge == "f32":
        m2 = ZincDCTransformer(**kw).to(gpu).train()
        m2(**feed)
        assert all(b.last_path == "composed" for b in m2.layers.blocks)


def _driver(tmp_path, tag, gpu, steps=3, discard=0, **kw):
    from egt_amd import training as T
    torch.manual_seed(0)
    cfg = dict(dict(scheme="zinc.svd", model_width=32, edge_width=32, batch_size=8, model_name=tag, num_epochs=1, initial_lr=1e-3,
                    use_svd=False, model_height=2, upto_hop=4, random_mask_prob=0.1, attn_dropout=0.1, fused_attn_dropout=True,
                    save_path=str(tmp_path / tag)), **kw)
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
    s.load_model()
    batch = next(iter(T.SyntheticZinc(8, 8, seed=1, pad_multiple=1)))
    blocks = [b for b in s.model.modules() if type(b).__name__ == "EGTBlock"]
    assert blocks and all(b.fused_attn_dropout and b.mha.attn_dropout == 0.1 for b in blocks)
    for _ in range(discard):                    # move every module's stream on by one sample
        for b in blocks:
            b.mha.next_seed()
    losses = []
    for step in range(steps):
        for b in blocks:
            b.last_path = None
        losses.append(s.train_step(batch))
        assert losses[-1] == losses[-1] and abs(losses[-1]) < float("inf"), losses
        assert all(b.last_path in (None, "fused") for b in blocks), [b.last_path for b in blocks]
    assert s.state.global_step == steps
    return s, losses, blocks


def test_zinc_svd_driver_eager_and_hipgraph_end_equal(tmp_path, gpu, egt_lib):
    """a zinc.svd config with attn_dropout 0.1, random_mask_prob 0.1 and the key, three train_steps of one geometry: eager (host
    seeds) and under use_hipgraph (device seeds, the second and third step are replays) draw the same masks and end with equal
    parameters.  The capture of a geometry runs one eager warm-up step whose sample is discarded (egt_amd.graph.GraphedStep), so
    the eager run discards one sample per module first: both runs then stand at the same place of every mask stream."""
    eager, le, be = _driver(tmp_path, "e", gpu, discard=1)
    assert all(b.last_path == "fused" for b in be)
    graphed, lg, bg = _driver(tmp_path, "g", gpu, use_hipgraph=True)
    assert graphed._seeds is not None and len(graphed._graphs) == 1 and all(b.last_path is None for b in bg)   # the last step was a replay
    assert le == lg, (le, lg)
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
    assert le[0] != le[1]                       # (the steps are not copies of each other: parameters and masks move)


def test_zinc_svd_driver_bf16_with_the_key(tmp_path, gpu, egt_lib):
    """... and the same config with bf16 edge tensors, which the composed route cannot run at all"""
    s, losses, blocks = _driver(tmp_path, "b", gpu, steps=2, edge_dtype="bf16")
    assert all(b.last_path == "fused" for b in blocks)


# ------------------------------------------------------------------------------------------- reference fixtures -----
@pytest.mark.parametrize("fix", list(AC.BLOCK_FIXTURES))
def test_block_vs_reference_fixture(fix, gpu, egt_lib):
    """the flagged kernels against what the reference's own model code computed (tests/golden/attn_dropout/<fix>.npz): the block is
    constructed with the fixture's seed, so its first training call draws the masks the reference was given"""
    inp, params, attrs, prob = AC.block_inputs(fix)
    c = dict(AC.BLOCK_SHAPE)
    blk = build(c, attrs, params, gpu, attrs["attn_dropout"], p=prob, seed=AC.BLOCK_SEED).train()
    out, dparams = run(blk, dict(inp, attn_mask=None), gpu)
    assert blk.last_path == "fused" and consumed_seed(blk) == AC.first_seed(AC.BLOCK_SEED)
    ref = AC.load_out(f"{fix}.npz")
    fixd = dict(h_out=ref["h_out"], e_out=ref["e_out"], dh=ref["dh"], de=ref["de"],
                dparams={k[2:]: v for k, v in ref.items() if k.startswith("d/")})
    compare(f"reference-{fix}", out, dparams, fixd)


def test_model_vs_reference_fixture(gpu, egt_lib):
    """ZincDCTransformer(attn_dropout=0.1, fused_attn_dropout=True) in training mode against the reference's DCSVDTransformer run
    (model_zinc*.npz): prediction, loss and every weight gradient, to the tolerances of tests/test_model.py's model cases; every
    block on the fused route, layer i drawing from the seed the fixture's i-th keep mask was made with"""
    from test_model import _load_params, _grad_of
    from egt_amd import ZincDCTransformer, mae_loss
    inp, params, cfg = AC.model_inputs()
    model = ZincDCTransformer(random_mask_prob=0.0, fused_attn_dropout=True, **cfg).to(gpu).train()
    _load_params(model, params, gpu)
    y = model(inp["node_features"].to(gpu), inp["feature_matrix"].to(gpu), inp["graph_matrix"].to(gpu))
    loss = mae_loss(y, inp["target"].to(gpu))
    loss.backward()
    assert all(b.last_path == "fused" for b in model.layers.blocks)
    assert [consumed_seed(b) for b in model.layers.blocks] == AC.model_seeds()
    ref = AC.load_out("model_zinc.npz", "model_zinc_grads.npz")
    assert_close(y, ref["y"], name="prediction", rtol=2e-4, arel=5e-5)
    assert_close(loss.reshape(1), ref["loss"], name="MAE", rtol=2e-4, arel=5e-5)
    dead = {id(p) for p in model._dead_edge_params()}
    checked = 0
    for k in params:
        prm = _grad_of(model, k)
        if prm is None:
            continue
        if id(prm) in dead:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, k
            continue
        assert_close(prm.grad, ref[f"d/{k}"], name=k, **BWD)
        checked += 1
    assert checked >= 14 * cfg["model_height"]
