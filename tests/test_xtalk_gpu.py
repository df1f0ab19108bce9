"""GPU parity of the cross-talk FFN (egt_amd.xtalk on csrc/egt_xtalk.hip) against the fp64 restatement of tests/xtalk_cases.py,
which tests/test_xtalk_cpu.py pins to the reference's own numbers.

Tolerance: util.FWD / util.BWD through util.assert_close, exactly as tests/test_ffn_gpu.py holds the channel FFN -- the
cross-talk FFN is the same two fp32 MFMA products per side, plus fp32 sums of at most N masked terms.
EGT_XTALK_MARGINS=<path>: the worst error / tolerance of every operator case is written there (JSON) when the module ends
(profiles/xtalk_margins.json is such a dump)."""
import json
import os

import numpy as np
import pytest
import torch

import reference_cases as RC
import virtual_nodes_ref as VR
import xtalk_cases as XC
from util import assert_close, margin, FWD, BWD

pytestmark = pytest.mark.gpu
MARGINS = {}
NAMES = XC.FFN_NAMES


@pytest.fixture(scope="module", autouse=True)
def _dump_margins():
    yield
    path = os.environ.get("EGT_XTALK_MARGINS")
    if path and MARGINS:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(tolerance="util.FWD (h_out, e_out) / util.BWD (gradients); margin = worst |error| / tolerance (< 1 passes)",
                           worst_margin=MARGINS), f, indent=1, sort_keys=True)


def _run(name, gpu, op):
    """one forward + backward of `op` on the case's fp32 tensors -> {tensor name: result}, named as XC.op_reference names them"""
    c, inp, pn, pe = XC.op_inputs(name)
    h, e = inp["h"].to(gpu).requires_grad_(), inp["e"].to(gpu).requires_grad_()
    pn = [pn[k].to(gpu).requires_grad_() for k in NAMES]
    pe = [pe[k].to(gpu).requires_grad_() for k in NAMES]
    h2, e2 = op(h, e, inp["mask"].to(gpu), pn, pe, c["n2e"], c["e2n"], c["act"])
    torch.autograd.backward([h2, e2], [inp["dh"].to(gpu), inp["de"].to(gpu)])
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=h.grad, de=e.grad)
    out.update({"node." + k: t.grad for k, t in zip(NAMES, pn)})
    out.update({"edge." + k: t.grad for k, t in zip(NAMES, pe)})
    return out


def _hold(name, got, tag):
    ref = XC.op_reference(name)
    assert set(got) == set(ref)
    worst = {}
    for k, r in ref.items():
        tol = FWD if k in ("h_out", "e_out") else BWD
        m = margin(got[k], r, rtol=tol["rtol"], arel=tol["arel"]) if float(r.abs().max()) >= 1e-9 else 0.0
        worst[k] = round(m, 4)
        print(f"{tag} {name} {k}: margin {m:.4f}")
    MARGINS[f"{tag}:{name}"] = dict(worst=max(worst.values()), where=max(worst, key=worst.get))
    for k, r in ref.items():
        assert_close(got[k], r, name=f"{name}: {k}", **(FWD if k in ("h_out", "e_out") else BWD))


@pytest.mark.parametrize("name", list(XC.OP_CASES))
def test_xtalk_ffn_vs_restatement(name, gpu, egt_lib):
    from egt_amd.xtalk import xtalk_ffn
    _hold(name, _run(name, gpu, xtalk_ffn), "fused")


@pytest.mark.parametrize("name", list(XC.OP_CASES))
def test_composed_fallback_vs_restatement(name, gpu, egt_lib):
    from egt_amd.xtalk import xtalk_ffn_composed
    _hold(name, _run(name, gpu, xtalk_ffn_composed), "composed")


@pytest.mark.parametrize("name", ["n33_de16_empty", "n37_de64", "n19_de32_relu", "n21_de64_sn64"])
def test_two_runs_are_bit_equal(name, gpu, egt_lib):
    from egt_amd.xtalk import xtalk_ffn
    a, b = _run(name, gpu, xtalk_ffn), _run(name, gpu, xtalk_ffn)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_empty_graph_gives_zero_exchange_and_finite_gradients(gpu, egt_lib):
    """divide_no_nan: graph 2 of n33_de16_empty has no node -- hn is 0 there, nothing is NaN, and d hn does not reach its edges"""
    from egt_amd import _lib as L
    from egt_amd.xtalk import _XtalkEdge, _desc, split_widths
    c, inp, pn, pe = XC.op_inputs("n33_de16_empty")
    s_e, s_n = split_widths(c["De"], c["Dh"], c["n2e"], c["e2n"])
    g = torch.Generator().manual_seed(1)
    hr, hc = (torch.randn(c["B"], c["N"], s_n, generator=g).to(gpu) for _ in range(2))
    e = inp["e"].to(gpu).requires_grad_()
    e2, hn = _XtalkEdge.apply(e, inp["mask"].to(gpu).float(), hr, hc, _desc(c["B"], c["N"], c["De"], c["Dh"], s_e, s_n, c["act"]),
                              *[pe[k].to(gpu) for k in NAMES])
    hv = hn.detach()
    assert torch.isfinite(hv).all() and float(hv[2].abs().max()) == 0.0 and float(hv[0].abs().max()) > 0
    hn.backward(torch.ones_like(hn))
    assert torch.isfinite(e.grad).all() and float(e.grad[2].abs().max()) == 0.0 and float(e.grad[0].abs().max()) > 0


def test_the_library_declines_and_the_op_says_so(gpu, egt_lib):
    from egt_amd.xtalk import xtalk_ffn, xtalk_supported
    assert not xtalk_supported(2, 9, 48, 48, 12, 12) and xtalk_supported(2, 9, 64, 64, 16, 48)
    c, inp, pn, pe = XC.op_inputs("n9_de16")
    with pytest.raises(ValueError, match="fused cross-talk FFN covers"):
        xtalk_ffn(inp["h"].to(gpu), inp["e"].to(gpu).bfloat16(), inp["mask"].to(gpu), [pn[k].to(gpu) for k in NAMES],
                  [pe[k].to(gpu) for k in NAMES], .25, .25)


# ------------------------------------------------------------------------------- reference fixtures end to end -----
@pytest.mark.parametrize("name", list(XC.MODEL_CASES))
def test_model_forward_backward_vs_reference(name, gpu, egt_lib):
    """prediction, loss and every parameter gradient of ZincDCTransformer with the keys on, against what the reference's model
    computed: the rule of tests/test_reference_golden_gpu.py (`close`)"""
    from egt_amd import ZincDCTransformer, mae_loss
    from test_reference_golden_gpu import check_digests, close, close_or_zero
    fix = XC.load(name)
    inp, params, cfg = XC.model_inputs(name)
    check_digests(fix, inp, params)
    model = ZincDCTransformer(random_mask_prob=0.0, **cfg).to(gpu).eval()
    named = model.keras_named_parameters()
    loaded = set()
    with torch.no_grad():
        for k, t in params.items():
            prm = VR.module_param(model, k)
            if prm is not None:                    # (edge_norm_final: readout_edges=False, the model has none)
                prm.copy_(t.to(gpu)); loaded.add(id(prm))
    assert {id(p) for p in named.values()} <= loaded
    dev = lambda k: inp[k].to(gpu)
    y = model(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
    assert model.layers.last_xtalk_route == "fused" and [b.last_path for b in model.layers.blocks] == ["fused"] * 2
    loss = mae_loss(y, dev("target"))
    loss.backward()
    close(fix, "y", y)
    close(fix, "loss", loss.reshape(1))
    _, _, mask = model.embeddings(dev("node_features"), dev("feature_matrix"), dev("graph_matrix"))
    assert np.array_equal(RC.sha(mask.to(torch.bool).cpu()), fix["sha"]["bits/node_mask"])
    live, checked = {id(p) for p in named.values()}, 0
    for k in params:
        prm = VR.module_param(model, k)
        if prm is None or id(prm) not in live:     # not a parameter of the Keras model: the reference's gradient is zero
            assert float(fix["stat"][f"d/{k}"][2]) == 0.0, f"{k}: the reference trains it, the model does not own it"
            assert prm is None or prm.grad is None or float(prm.grad.abs().max()) == 0.0, k
            continue
        close_or_zero(fix, f"d/{k}", prm.grad); checked += 1
    assert checked == len(named)


# ------------------------------------------------------------------------------------------------ training -----
def _zinc_run(tag, graph, tmp_path, gpu, epochs=2, **kw):
    import egt_amd.training as T
    torch.manual_seed(0)
    cfg = dict(scheme="zinc.svd", model_width=64, edge_width=16, batch_size=8, model_name=tag, num_epochs=epochs, initial_lr=2e-3,
               use_svd=False, model_height=2, upto_hop=4, random_mask_prob=0.0, use_hipgraph=graph, save_path=str(tmp_path / tag),
               node2edge_xtalk=.25, edge2node_xtalk=.25, **kw)
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
    s.execute_training(T.SyntheticZinc(32, 8, seed=1, pad_multiple=1), T.SyntheticZinc(16, 8, seed=2, pad_multiple=1))
    return s


def test_two_epochs_reduce_the_loss_and_hipgraph_equals_eager(tmp_path, gpu, egt_lib):
    eager = _zinc_run("e", False, tmp_path, gpu)
    assert eager.model.layers.xtalk == (.25, .25) and eager.model.layers.last_xtalk_route == "fused"
    assert tuple(eager.model.layers.ffn_edge[0].lr2_kernel.shape) == (40, 16)
    losses = [h["loss"] for h in eager.history]
    assert len(losses) == 2 and losses[1] < losses[0], losses
    graphed = _zinc_run("g", True, tmp_path, gpu)
    assert len(graphed._graphs) >= 1
    assert [h["loss"] for h in graphed.history] == losses
    for a, b in zip(eager.params, graphed.params):
        assert torch.equal(a, b)
