"""Degree scalers (scale_degree, EGT_BF_SCALE_DEGREE) on the fused block: forward, backward and the fourteen parameter gradients
of the SD instances of the MFMA-tile pair kernels against the fp64 oracle (oracle.egt_oracle.block_forward(..., scale_degree=True)),
under the suite's FWD / BWD, compared as tests/test_block_gpu.py compares them.  Which kernels a shape reaches is asserted through
egt_block_launch_form / egt_block_bwd_kernel, so a plan change cannot hide a family.

EGT_SCALE_DEGREE_MARGINS=<path>: the worst error / tolerance of every parity case is written there (JSON) when the module ends."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import cases as CS
from scale_degree_cases import SHAPES, make_case, oracle
from test_block_gpu import PMAP
from util import assert_close, margin, FWD, BWD

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = "tests/" + os.path.basename(__file__)
MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    path = os.environ.get("EGT_SCALE_DEGREE_MARGINS")
    if path and MARGINS:
        old = {}
        if os.path.exists(path):      # (the child runs of this module add their cases to the parent's file)
            try:
                old = json.load(open(path))
            except ValueError:
                old = {}
        old.update(MARGINS)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def want_path():
    from egt_amd import fused as FZ
    return "composed" if FZ.scale_degree_disabled() else "fused"


def build(c, attrs, params, dev, scaler, fused="auto", p=0.0):
    from egt_amd import EGTBlock
    blk = EGTBlock(model_width=c["Dh"], edge_width=c["De"], num_heads=8, gate_attention=True,
                   edge_channel_type=attrs["edge_channel_type"], scale_degree=True, scaler_type=scaler,
                   random_mask_prob=p, fused=fused).to(dev)
    with torch.no_grad():
        for k, (m, a) in PMAP.items():
            if hasattr(blk, m):
                getattr(getattr(blk, m), a).copy_(params[k].to(dev))
    return blk


def run(blk, inp, dev, rand_mask=None):
    cu = lambda t: None if t is None else t.to(dev)
    h = cu(inp["h"]).requires_grad_(); e = cu(inp["e"]).requires_grad_()
    h2, e2 = blk(h, e, cu(inp["mask"]), cu(inp["attn_mask"]), rand_mask=cu(rand_mask))
    ((h2 * cu(inp["dh"])).sum() + (e2 * cu(inp["de"])).sum()).backward()
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad)
    dparams = {k: getattr(getattr(blk, m), a).grad for k, (m, a) in PMAP.items() if hasattr(blk, m)}
    return out, dparams


def compare(tag, out, dparams, ref, bias=False):
    ref = dict(ref)
    rd = ref.pop("dparams")
    m = {}
    for k, tol in (("h_out", FWD), ("e_out", FWD), ("dh", BWD), ("de", BWD)):
        if bias and k == "e_out":
            continue
        m[k] = margin(out[k], ref[k], rtol=tol["rtol"], arel=tol["arel"])
    for k, g in rd.items():
        if g is not None and float(g.abs().max()) >= 1e-9:
            m[k] = margin(dparams[k], g, rtol=BWD["rtol"], arel=BWD["arel"])
    MARGINS[tag] = dict(worst=max(m.values()), by_tensor=m)
    print(f"[scale_degree margins] {tag}: worst {max(m, key=m.get)} {max(m.values()):.3f}")
    assert_close(out["h_out"], ref["h_out"], name="h_out", **FWD)
    if not bias:
        assert_close(out["e_out"], ref["e_out"], name="e_out", **FWD)
    assert_close(out["dh"], ref["dh"], name="dh", **BWD)
    assert_close(out["de"], ref["de"], name="de", **BWD)
    for k, g in rd.items():
        if g is None:
            assert dparams.get(k) is None or float(dparams[k].abs().max()) == 0.0, k
            continue
        assert_close(dparams[k], g, name=k, **BWD)


def forms(egt_lib, blk, B, N, training=False):
    from egt_amd import fused as FZ
    desc = FZ._desc(blk, B, N, training, 0)
    assert egt_lib.egt_block_supported(C.byref(desc)) == 1
    return egt_lib.egt_block_launch_form(C.byref(desc)).decode(), egt_lib.egt_block_bwd_kernel(C.byref(desc)).decode()


PARITY = [(s, t) for s in SHAPES for t in ("log", "linear") if not (s == "n150_d4_de8" and t == "linear")]


def parity(shape, scaler, gpu, egt_lib, tag=None, **kw):
    B, N, d, De, nodes, ffwd, fbwd = SHAPES[shape]
    inp, params, attrs, c = make_case(B, N, d, De, nodes, shape, **kw)
    blk = build(c, attrs, params, gpu, scaler).eval()
    form, bk = forms(egt_lib, blk, B, N)
    out, dparams = run(blk, inp, gpu)
    assert blk.last_path == want_path()
    if not (os.environ.get("EGT_BWD_TL") or os.environ.get("EGT_FWD_ROWS")):
        assert f"fwd={ffwd}" in form and f"bwd={fbwd}/" in form and bk == fbwd, (form, bk)
    else:
        assert fbwd in form and bk == fbwd, (form, bk)
    compare(tag or f"{shape}-{scaler}", out, dparams, oracle(inp, params, attrs, scaler))


@pytest.mark.parametrize("shape,scaler", PARITY)
def test_block_vs_oracle(shape, scaler, gpu, egt_lib):
    parity(shape, scaler, gpu, egt_lib)


@pytest.mark.parametrize("shape", ["n19_de64", "n69_de8"])
@pytest.mark.parametrize("scaler", ["log", "linear"])
def test_small_degree(shape, scaler, gpu, egt_lib):
    """head 0's gate bias is -12: its degree is 1e-5 .. 1e-3 on every row (tests/test_scale_degree_cpu.py pins the recipe), where
    log(1 + deg) evaluated as __logf(1 + deg) has lost the digits log1pf keeps"""
    parity(shape, scaler, gpu, egt_lib, tag=f"small-{shape}-{scaler}", gate_bias0=-12.0)


@pytest.mark.parametrize("shape,N,d,De", [("constrained_n19_de64", 19, 8, 64), ("constrained_n37_d6_de48", 37, 6, 48)])
@pytest.mark.parametrize("scaler", ["log", "linear"])
def test_constrained_attention_mask(shape, N, d, De, scaler, gpu, egt_lib):
    """the mask-tensor instances: k_block_fwd<.., ML> and k_block_bwd_v4<.., ML>"""
    inp, params, attrs, c = make_case(2, N, d, De, [N, N - 6], shape, ect="constrained")
    blk = build(c, attrs, params, gpu, scaler).eval()
    form, bk = forms(egt_lib, blk, 2, N)
    assert "fwd=k_block_fwd/" in form and bk == "k_block_bwd_v4", (form, bk)
    out, dparams = run(blk, inp, gpu)
    assert blk.last_path == want_path()
    compare(f"{shape}-{scaler}", out, dparams, oracle(inp, params, attrs, scaler))


@pytest.mark.parametrize("shape", ["n19_de64", "n69_de8"])
def test_injected_random_mask(shape, gpu, egt_lib):
    """a host random-mask tensor in training mode (the ML instances again, De = 8 included): the degree leaves the masked keys out"""
    B, N, d, De, nodes, _, _ = SHAPES[shape]
    inp, params, attrs, c = make_case(B, N, d, De, nodes, shape + "rm", rand_p=0.3)
    blk = build(c, attrs, params, gpu, "log", p=0.3).train()
    out, dparams = run(blk, inp, gpu, rand_mask=inp["rand_mask"])
    assert blk.last_path == want_path()
    compare(f"injected-rm-{shape}", out, dparams, oracle(inp, params, attrs, "log", rand_mask=inp["rand_mask"]))


@pytest.mark.parametrize("shape,scaler", [("n19_de64", "log"), ("n37_d6_de48", "linear"), ("n80_de16", "log"), ("n69_de8", "linear")])
def test_in_kernel_random_mask(shape, scaler, gpu, egt_lib):
    """training mode, random_mask_prob 0.3, the kernels' own sample (egt_mask_sample's stream, replicated by oracle.rng_ref): the
    degree excludes the randomly masked keys in both directions"""
    from oracle import rng_ref
    B, N, d, De, nodes, _, fbwd = SHAPES[shape]
    p = 0.3
    inp, params, attrs, c = make_case(B, N, d, De, nodes, shape + "ik")
    blk = build(c, attrs, params, gpu, scaler, p=p).train()
    form, bk = forms(egt_lib, blk, B, N, training=True)
    assert bk == fbwd, (form, bk)            # (the in-kernel mask is no mask tensor: the plan stays)
    out, dparams = run(blk, inp, gpu)
    assert blk.last_path == want_path()
    seed = (blk.mha.seed * 0x9E3779B97F4A7C15 + blk.mha._calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    rm = torch.from_numpy(rng_ref.random_mask(seed, B, N, 8, p))
    compare(f"in-kernel-rm-{shape}-{scaler}", out, dparams, oracle(inp, params, attrs, scaler, rand_mask=rm))


@pytest.mark.parametrize("shape", ["n19_de64", "n69_de8"])
def test_zero_degree_graph(shape, gpu, egt_lib):
    """one graph of the batch has no real node: deg = 0 on its rows, s = 0, V_att' = 0, every gradient finite (no 0 / 0); the
    other graphs come out as in the call without it -- to the bit where both calls have the same launch form (a graph's rows are
    computed by workgroups of their own, in the same order of operations), within FWD / BWD otherwise"""
    B, N, d, De, nodes, _, _ = SHAPES[shape]
    inp, params, attrs, c = make_case(3, N, d, De, [N, 0, N - 5], shape + "zero")
    blk = build(c, attrs, params, gpu, "log").eval()
    out, dparams = run(blk, inp, gpu)
    assert blk.last_path == want_path()
    for k, v in list(out.items()) + list(dparams.items()):
        assert torch.isfinite(v).all(), k
    compare(f"zero-degree-{shape}", out, dparams, oracle(inp, params, attrs, "log"))
    keep = [0, 2]
    inp2 = {k: (v[keep] if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    blk.zero_grad()
    out2, _ = run(blk, inp2, gpu)
    same_form = blk.last_path == "fused" and forms(egt_lib, blk, 3, N) == forms(egt_lib, blk, 2, N)
    print(f"[zero degree] {shape}: launch form with and without the empty graph {'the same: bit equality' if same_form else 'differs: FWD / BWD'}")
    for k, tol in (("h_out", FWD), ("e_out", FWD), ("dh", BWD), ("de", BWD)):
        if same_form:
            assert torch.equal(out[k][keep], out2[k]), f"{k} without the empty graph: {int((out[k][keep] != out2[k]).sum())} elements differ"
        else:
            assert_close(out[k][keep], out2[k], name=f"{k} without the empty graph", **tol)


@pytest.mark.parametrize("scaler", ["log", "linear"])
def test_bias_edge_channels_de8(scaler, gpu, egt_lib):
    """'bias' edge channels at De = 8 with degree scalers: the per-layer-bias route on r4 / v4r (the static-edge kernels have no degree)"""
    inp, params, attrs, c = make_case(2, 21, 8, 8, [21, 15], "bias_sd", ect="bias")
    blk = build(c, attrs, params, gpu, scaler).eval()
    blk._static_edge = True            # as inside an EGTLayerStack: still never "static"
    out, dparams = run(blk, inp, gpu)
    assert blk.last_path == want_path()
    if blk.last_path == "fused":
        assert blk.last_edge_route == "per-layer-bias"
    compare(f"bias-de8-{scaler}", out, dparams, oracle(inp, params, attrs, scaler), bias=True)


def test_ungated_refusal():
    from egt_amd import EGTBlock
    with pytest.raises(ValueError, match="gate_attention"):
        EGTBlock(gate_attention=False, scale_degree=True)


# ---------------------------------------------------------------------------------------- launch-plane overrides -----
def _child(env, select):
    e = dict(os.environ, **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", HERE, "-k", select],
                       cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


@pytest.mark.skipif(bool(os.environ.get("EGT_SD_CHILD")), reason="a child run does not start children")
@pytest.mark.parametrize("env,select", [({"EGT_BWD_TL": "4"}, "test_block_vs_oracle and n69_de64-log"),
                                        ({"EGT_FWD_ROWS": "4"}, "test_block_vs_oracle and n37_d6_de48-linear"),
                                        ({"EGT_NO_SCALE_DEGREE": "1"}, "test_block_vs_oracle and (n19_de64 or n69_de8)")],
                         ids=["bwd_tl4", "fwd_rows4", "composed_route"])
def test_child_process_switches(env, select, gpu):
    """EGT_BWD_TL / EGT_FWD_ROWS / EGT_NO_SCALE_DEGREE are read once per process: the parity cases again in a child (the last one:
    last_path == 'composed', same numbers within tolerance -- want_path())"""
    _child(dict(env, EGT_SD_CHILD="1"), select)


# --------------------------------------------------------------------------------------------- existing behaviour -----
def _raw_block(egt_lib, gpu, flags_extra, poison_slot3):
    """egt_block_fwd / egt_block_bwd through the C ABI at [2, 19, 64], De = 64; -> (h_out, e_out, d_h, d_e, saved as floats)"""
    from egt_amd import _lib as L
    import memcontract as M
    row = ("sd_raw", 2, 19, 8, 64, False, "", "", "")
    inp = M.block_inputs(row)
    desc = M.block_desc(row)
    desc.flags |= flags_extra
    p = C.byref(desc)
    dev = lambda t: t.to(gpu).contiguous()
    h, e, km, dh, de = dev(inp["h"]), dev(inp["e"]), dev(inp["key_mask"]), dev(inp["dh"]), dev(inp["de"])
    prm = [dev(t) for t in inp["params"][0]]
    grd = [torch.empty_like(t) for t in prm]
    saved = torch.zeros(egt_lib.egt_block_saved_bytes(p) // 4, device=gpu)
    ws = torch.zeros(egt_lib.egt_block_workspace_bytes(p), dtype=torch.uint8, device=gpu)
    h_out, e_out, d_h, d_e = torch.empty_like(h), torch.empty_like(e), torch.empty_like(h), torch.empty_like(e)
    ps = L.params_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, prm)
    gs = L.params_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, grd)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L.check(egt_lib.egt_block_fwd(p, C.byref(ps), ptr(h), ptr(e), ptr(km), None, None, ptr(h_out), ptr(e_out), ptr(saved), ptr(ws),
                                  L.current_stream()))
    if poison_slot3:      # the statistics [B N, 8, 4] follow V_att [B N Dh] (64-float aligned) in `saved`
        rows = 2 * 19
        off = (rows * 64 + 63) // 64 * 64
        saved[off:off + rows * 32].view(rows * 8, 4)[:, 3] = float("nan")
    L.check(egt_lib.egt_block_bwd(p, C.byref(ps), ptr(h), ptr(e), ptr(km), None, None, ptr(saved), ptr(dh), ptr(de), ptr(d_h), ptr(d_e),
                                  C.byref(gs), ptr(ws), L.current_stream()))
    torch.cuda.synchronize()
    return [h_out, e_out, d_h, d_e] + grd


def test_unflagged_block_never_reads_slot3(gpu, egt_lib):
    """a block WITHOUT the flag: slot 3 of its saved statistics pre-filled with NaN between forward and backward changes no bit of any
    output (the unflagged kernels neither write nor read it)"""
    a = _raw_block(egt_lib, gpu, 0, False)
    b = _raw_block(egt_lib, gpu, 0, True)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(y).all(), i
        assert torch.equal(x, y), i


def test_flag_changes_the_block(gpu, egt_lib):
    """... and the same call with the flag is another function of its inputs (the flag reaches the kernels)"""
    from egt_amd import _lib as L
    a = _raw_block(egt_lib, gpu, 0, False)
    b = _raw_block(egt_lib, gpu, L.BF_SCALE_DEGREE, False)
    assert not torch.equal(a[0], b[0]) and torch.isfinite(b[0]).all()
    assert torch.equal(a[1], b[1])            # e' does not depend on the degree


# --------------------------------------------------------------------------------------------------- model / driver -----
@pytest.mark.parametrize("scaler", ["log", "linear"])
def test_zinc_model_takes_the_fused_route(scaler, gpu, egt_lib):
    """ZincDCTransformer(scale_degree=True) in training mode with the in-kernel random mask: every block on the fused route, and the
    same model on the composed route (fused='off' blocks) gives the same prediction and gradients in eval mode"""
    from egt_amd.model import ZincDCTransformer
    torch.manual_seed(5)
    kw = dict(model_width=64, edge_width=16, model_height=2, upto_hop=4, scale_degree=True, scaler_type=scaler)
    m = ZincDCTransformer(random_mask_prob=0.1, **kw).to(gpu)
    inp, _, c = CS.make_model_case("zinc_small")
    feed = {k: v.to(gpu) for k, v in inp.items() if k != "target"}
    m.train()
    y = m(**feed)
    y.sum().backward()
    blocks = [b for b in m.modules() if type(b).__name__ == "EGTBlock"]
    assert blocks and all(b.last_path == "fused" for b in blocks)
    assert torch.isfinite(y).all() and all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    m.eval(); m.zero_grad()
    y1 = m(**feed); y1.sum().backward()
    g1 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    for b in blocks:
        b.fused = "off"
    m.zero_grad()
    y2 = m(**feed); y2.sum().backward()
    assert all(b.last_path == "composed" for b in blocks)
    assert_close(y1, y2, name="prediction fused vs composed", rtol=2e-4, arel=5e-5)
    # two fp32 routes against each other: twice BWD.  d(dense_edge_b.bias) is analytically zero (the softmax does not see a shift of
    # a row's logits) and rounding noise on both routes: its absolute term is relative to the gate bias gradient's magnitude
    floor = {n: float(p.grad.abs().max()) for n, p in m.named_parameters() if n.endswith("attention_gates.bias")}
    for n, p in m.named_parameters():
        if p.grad is not None:
            fl = floor[n.replace("dense_edge_b", "attention_gates")] if n.endswith("dense_edge_b.bias") else 0.0
            assert_close(g1[n], p.grad, name=n, rtol=2e-3, arel=2e-4, floor=fl)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_zinc_svd_scheme_trains_on_the_fused_route(graph, tmp_path, gpu, egt_lib):
    """a zinc.svd config with "scale_degree": true on a synthetic batch: two `train_step`s of the same geometry with the in-kernel
    random mask, eager and under use_hipgraph (the second graphed step is the cached graph's replay: the batch copied into the static
    tensors, the device seeds advanced); after each step the loss is finite and every block is on the fused route"""
    from egt_amd import training as T
    torch.manual_seed(0)
    cfg = dict(scheme="zinc.svd", model_width=32, edge_width=32, batch_size=8, model_name="sd", num_epochs=1, initial_lr=1e-3,
               use_svd=False, model_height=2, upto_hop=4, random_mask_prob=0.1, scale_degree=True, use_hipgraph=graph,
               save_path=str(tmp_path / "sd"))
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
    s.load_model()
    batch = next(iter(T.SyntheticZinc(8, 8, seed=1, pad_multiple=1)))
    blocks = [b for b in s.model.modules() if type(b).__name__ == "EGTBlock"]
    assert blocks and all(b.mha.scale_degree for b in blocks)
    losses = []
    for step in range(2):
        for b in blocks:
            b.last_path = None
        losses.append(s.train_step(batch))
        assert losses[-1] == losses[-1] and abs(losses[-1]) < float("inf"), losses
        assert all(p is None or bool(torch.isfinite(p).all()) for p in (q.grad for q in s.params))
        if graph and step == 1:      # the cached graph was replayed: no Python forward ran, the route is the captured one
            assert len(s._graphs) == 1 and all(b.last_path is None for b in blocks)
        else:
            assert all(b.last_path == "fused" and b.training for b in blocks), [b.last_path for b in blocks]
    assert s.state.global_step == 2
    if graph:
        assert s._seeds is not None


# ------------------------------------------------------------------------------------------- reference fixtures -----
@pytest.mark.parametrize("scaler", ["log", "linear"])
def test_block_vs_reference_fixture(scaler, gpu, egt_lib):
    """the fused block against what the reference's own model code computed (tests/golden/scale_degree/block_<scaler>.npz)"""
    import scale_degree_cases as SC
    inp, params, attrs = SC.block_inputs(scaler)
    c = dict(SC.BLOCK_SHAPE)
    blk = build(c, attrs, params, gpu, scaler).eval()
    out, dparams = run(blk, inp, gpu)
    assert blk.last_path == want_path()
    ref = SC.load_out(f"block_{scaler}.npz")
    fix = dict(h_out=ref["h_out"], e_out=ref["e_out"], dh=ref["dh"], de=ref["de"],
               dparams={k[2:]: v for k, v in ref.items() if k.startswith("d/")})
    compare(f"reference-block-{scaler}", out, dparams, fix)


def test_model_vs_reference_fixture(gpu, egt_lib):
    """ZincDCTransformer(scale_degree=True) against the reference's DCSVDTransformer run (model_zinc*.npz): prediction, loss and
    every weight gradient, to the tolerances of tests/test_model.py's model cases; every block on the fused route"""
    import scale_degree_cases as SC
    from test_model import _load_params, _grad_of
    from egt_amd import ZincDCTransformer, mae_loss
    inp, params, cfg = SC.model_inputs()
    model = ZincDCTransformer(random_mask_prob=0.0, **cfg).to(gpu).eval()
    _load_params(model, params, gpu)
    y = model(inp["node_features"].to(gpu), inp["feature_matrix"].to(gpu), inp["graph_matrix"].to(gpu))
    loss = mae_loss(y, inp["target"].to(gpu))
    loss.backward()
    assert all(b.last_path == want_path() for b in model.layers.blocks)
    ref = SC.load_out("model_zinc.npz", "model_zinc_grads.npz")
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
