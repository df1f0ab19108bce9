"""Cases of the cross-talk FFN (node2edge_xtalk / edge2node_xtalk, lib/models/graph_xformer_model_base.py:227-324): an fp64
restatement of the exchange, the operator cases of tests/test_xtalk_gpu.py, and the model cases whose reference numbers --
the reference's own ZINC model executed in fp64 through oracle.ref_exec -- live in tests/golden/xtalk/*.npz
(tests/golden/make_xtalk_golden.py writes them; the fixture format is that of tests/reference_cases.py).

No test functions here."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

import cases as CS
import reference_cases as RC
from oracle import egt_model_oracle as MO, egt_oracle as O, ref_exec as RX

XT_DIR = os.path.join(CS.GOLDEN_DIR, "xtalk")
F64 = torch.float64
FFN_NAMES = CS.FFN_NAMES
H = 8


def widths(De, Dh, n2e, e2n, mult=2.0):
    """(s_e, s_n, lr2 input width of the node side, of the edge side): graph_xformer_model_base.py:270-271, :286-287"""
    he, hn = round(De * mult), round(Dh * mult)
    s_e = round(e2n * he / mult) if e2n > 0 else 0
    s_n = round(n2e * hn / mult) if n2e > 0 else 0
    return s_e, s_n, hn - 2 * s_n + s_e, he - 2 * s_e + s_n


def _act(x, act):
    return torch.nn.functional.elu(x) if act == "elu" else torch.relu(x)


def xtalk_ffn_ref(h, e, mask, pn, pe, n2e, e2n, act="elu"):
    """ffn_block with cross-talk (:309-324 around channel_xtalk :260-307), index by index.  pn / pe: the six FFN tensors of the
    node / edge side by FFN_NAMES; mask [B,N] bool."""
    s_e, s_n, _, _ = widths(e.shape[-1], h.shape[-1], n2e, e2n)
    xn = O.dense(O.layer_norm(h, pn["norm_gamma"], pn["norm_beta"]), pn["lr1_kernel"], pn["lr1_bias"])   # no activation: xtalk_flag
    xe = O.dense(O.layer_norm(e, pe["norm_gamma"], pe["norm_beta"]), pe["lr1_kernel"], pe["lr1_bias"])
    m = mask.to(h.dtype)
    hn = en = None
    if e2n > 0:
        er, ec, xe = xe[..., :s_e], xe[..., s_e:2 * s_e], xe[..., 2 * s_e:]
        r = torch.einsum("bi,bijc->bjc", m, er)          # reduce_sum(x_er * m[:, :, None, None], axis=1)
        c = torch.einsum("bj,bijc->bic", m, ec)          # reduce_sum(x_ec * m[:, None, :, None], axis=2)
        cnt = m.sum(dim=1)[:, None, None]
        hn = torch.where(cnt != 0, (r + c) / torch.where(cnt != 0, cnt, torch.ones_like(cnt)), torch.zeros_like(r))   # divide_no_nan
    if n2e > 0:
        hr, hc, xn = xn[..., :s_n], xn[..., s_n:2 * s_n], xn[..., 2 * s_n:]
        en = hr[:, :, None, :] + hc[:, None, :, :]
    if hn is not None:
        xn = torch.cat([xn, hn], dim=-1)
    if en is not None:
        xe = torch.cat([xe, en], dim=-1)
    return (h + O.dense(_act(xn, act), pn["lr2_kernel"], pn["lr2_bias"]),
            e + O.dense(_act(xe, act), pe["lr2_kernel"], pe["lr2_bias"]))


def xtalk_edge_ref(e, mask, hr, hc, pe, s_e, s_n, act="elu"):
    """the edge side alone, as egt_xtalk_fwd states it: (e, mask, hr, hc) -> (e', hn); hr / hc None with s_n = 0, hn None with s_e = 0"""
    xe = O.dense(O.layer_norm(e, pe["norm_gamma"], pe["norm_beta"]), pe["lr1_kernel"], pe["lr1_bias"])
    m = mask.to(e.dtype)
    hn = None
    if s_e:
        cnt = m.sum(dim=1)[:, None, None]
        tot = torch.einsum("bi,bijc->bjc", m, xe[..., :s_e]) + torch.einsum("bj,bijc->bic", m, xe[..., s_e:2 * s_e])
        hn = torch.where(cnt != 0, tot / torch.where(cnt != 0, cnt, torch.ones_like(cnt)), torch.zeros_like(tot))
    z = xe[..., 2 * s_e:]
    if s_n:
        z = torch.cat([z, hr[:, :, None, :] + hc[:, None, :, :]], dim=-1)
    return e + O.dense(_act(z, act), pe["lr2_kernel"], pe["lr2_bias"]), hn


# ------------------------------------------------------------------------------------------ operator cases -----
# (B, N, De, Dh), node counts, fractions, activation.  N = 9: one ragged tile; 19 / 33 / 37: ragged last tiles and three / five
# row blocks of eight rows per graph, i.e. two workgroups per graph at 33 and 37 (column partials cross workgroups); a graph
# without nodes (divide_no_nan); each one-sided fraction; relu; no, one, two, three and four exchange tiles of 16 channels.
OP_CASES = {
    "n9_de16": dict(B=2, N=9, De=16, Dh=64, nodes=(9, 6), n2e=.25, e2n=.25, act="elu"),
    "n19_de32_n2e": dict(B=2, N=19, De=32, Dh=64, nodes=(19, 11), n2e=.25, e2n=0., act="elu"),
    "n19_de32_relu": dict(B=2, N=19, De=32, Dh=64, nodes=(19, 11), n2e=.5, e2n=.25, act="relu"),
    "n37_de64": dict(B=1, N=37, De=64, Dh=48, nodes=(29,), n2e=.25, e2n=.25, act="relu"),
    "n37_de64_e2n": dict(B=1, N=37, De=64, Dh=48, nodes=(29,), n2e=0., e2n=.5, act="elu"),
    "n33_de16_empty": dict(B=3, N=33, De=16, Dh=64, nodes=(33, 17, 0), n2e=.25, e2n=.25, act="elu"),
    # De = 64 with three and four exchange tiles: the backward takes the exchange rows of d fnn_lr2_edge in its second walk
    "n37_de64_sn48": dict(B=1, N=37, De=64, Dh=64, nodes=(31,), n2e=.75, e2n=.25, act="elu"),
    "n21_de64_sn64": dict(B=2, N=21, De=64, Dh=64, nodes=(21, 13), n2e=1., e2n=.25, act="relu"),
}


def ffn_params(W, lr2_in, g, prefix=""):
    hid = 2 * W
    lim1, lim2 = (6.0 / (W + hid)) ** 0.5, (6.0 / (lr2_in + W)) ** 0.5
    return {prefix + "norm_gamma": 1.0 + 0.3 * torch.randn(W, generator=g), prefix + "norm_beta": 0.3 * torch.randn(W, generator=g),
            prefix + "lr1_kernel": (torch.rand(W, hid, generator=g) * 2 - 1) * lim1, prefix + "lr1_bias": 0.2 * torch.randn(hid, generator=g),
            prefix + "lr2_kernel": (torch.rand(lr2_in, W, generator=g) * 2 - 1) * lim2, prefix + "lr2_bias": 0.2 * torch.randn(W, generator=g)}


def op_inputs(name):
    """-> (case, {h, e, mask, dh, de}, node params, edge params): fp32 tensors of a seeded recipe"""
    c = OP_CASES[name]
    g = torch.Generator().manual_seed(4100 + sum(map(ord, name)))
    B, N, De, Dh = c["B"], c["N"], c["De"], c["Dh"]
    _, _, kn, ke = widths(De, Dh, c["n2e"], c["e2n"])
    mask = torch.arange(N)[None, :] < torch.tensor(c["nodes"])[:, None]
    inp = dict(h=torch.randn(B, N, Dh, generator=g) * 1.5 + 0.2, e=torch.randn(B, N, N, De, generator=g) * 1.5 + 0.2, mask=mask,
               dh=torch.randn(B, N, Dh, generator=g), de=torch.randn(B, N, N, De, generator=g))
    return c, inp, ffn_params(Dh, kn, g), ffn_params(De, ke, g)


@functools.lru_cache(maxsize=None)
def op_reference(name):
    """fp64: h', e' and the gradients of sum(h' dh) + sum(e' de) w.r.t. h, e and the twelve parameters.  Computed once."""
    c, inp, pn, pe = op_inputs(name)
    h, e = inp["h"].to(F64).requires_grad_(), inp["e"].to(F64).requires_grad_()
    pn64 = {k: v.to(F64).requires_grad_() for k, v in pn.items()}
    pe64 = {k: v.to(F64).requires_grad_() for k, v in pe.items()}
    h2, e2 = xtalk_ffn_ref(h, e, inp["mask"], pn64, pe64, c["n2e"], c["e2n"], c["act"])
    leaves = [h, e] + [pn64[k] for k in FFN_NAMES] + [pe64[k] for k in FFN_NAMES]
    gr = torch.autograd.grad([h2, e2], leaves, [inp["dh"].to(F64), inp["de"].to(F64)])
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=gr[0], de=gr[1])
    out.update({"node." + k: t for k, t in zip(FFN_NAMES, gr[2:8])})
    out.update({"edge." + k: t for k, t in zip(FFN_NAMES, gr[8:])})
    return out


# --------------------------------------------------------------------------------------------- model cases -----
# the reference's ZINC model, B = 2, N = 9 (9 and 6 nodes), width 64, height 2; hidden widths 40/100, 48/96, 16/136 at De = 16
FRACTIONS = {"both": (.25, .25), "n2e": (.25, 0.), "e2n": (0., .5)}
MODEL_CASES = {f"de{De}_{f}": dict(De=De, n2e=FRACTIONS[f][0], e2n=FRACTIONS[f][1], ect="residual")
               for De in (16, 32) for f in FRACTIONS}
MODEL_CASES["de16_both_constrained"] = dict(De=16, n2e=.25, e2n=.25, ect="constrained")
MODEL_CAP = 128


def model_inputs(name):
    """-> (inputs, fp32 parameters under the oracle's keys, model config)"""
    c = MODEL_CASES[name]
    cfg = dict(model_width=64, edge_width=c["De"], model_height=2, upto_hop=4, edge_channel_type=c["ect"],
               node2edge_xtalk=c["n2e"], edge2node_xtalk=c["e2n"])
    g = torch.Generator().manual_seed(5200 + sum(map(ord, name)))
    B, N = 2, 9
    n = torch.tensor([9, 6])
    real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.randint(0, 28, (B, N), generator=g)
    nf[~real] = -1
    adj = (torch.rand(B, N, N, generator=g) > 0.6).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float() * (1 - torch.eye(N))[None]
    fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
    inp = dict(node_features=nf, feature_matrix=fm, graph_matrix=adj, target=torch.randn(B, 1, generator=g))
    p = MO.init_zinc_params(cfg, dtype=torch.float32, generator=g)
    _, _, kn, ke = widths(c["De"], 64, c["n2e"], c["e2n"])
    for ii in range(cfg["model_height"]):   # fnn_lr2 at the exchanged widths
        for tag, W, k in (("node", 64, kn), ("edge", c["De"], ke)):
            lim = (6.0 / (k + W)) ** 0.5
            p[f"layer{ii}.ffn_{tag}.lr2_kernel"] = (torch.rand(k, W, generator=g) * 2 - 1) * lim
    return inp, p, cfg


def model_forward(inp, p, cfg):
    """MO.zinc_forward with the cross-talk ffn_block in its layer loop -> (y, node mask, edge mask or None)"""
    act, adj = cfg.get("activation", "elu"), inp["graph_matrix"]
    h, e, mask = MO.zinc_embeddings(inp["node_features"], inp["feature_matrix"], adj, p, cfg)
    M = O.constrained_edge_mask(adj.to(h.dtype), H) if cfg["edge_channel_type"] == "constrained" else None
    for ii in range(cfg["model_height"]):
        bp = {k[len(f"layer{ii}."):]: v for k, v in p.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
        h, e = O.block_forward(h, e, mask, bp, num_heads=H, attn_mask=M)
        fn = {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_node.")}
        fe = {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_edge.")}
        h, e = xtalk_ffn_ref(h, e, mask, fn, fe, cfg["node2edge_xtalk"], cfg["edge2node_xtalk"], act)
    h = O.layer_norm(h, p["node_norm_final.gamma"], p["node_norm_final.beta"])
    x = MO.mlp_out(MO.masked_global_avg_pool_1d(h, mask), p, 2, act)
    return O.dense(x, p["target.kernel"], p["target.bias"]), mask, M


def oracle_model(name):
    """fp64 restatement -> ({y, loss, d/<parameter>}, {node_mask[, edge_mask]})"""
    inp, params, cfg = model_inputs(name)
    p = {k: t.to(F64).requires_grad_() for k, t in params.items()}
    y, mask, M = model_forward(inp, p, cfg)
    loss = MO.mae_loss(y, inp["target"].to(F64))
    gr = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    out = dict(y=y.detach(), loss=loss.detach().reshape(1))
    out.update({f"d/{k}": (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(p, gr)})
    bits = dict(node_mask=mask)
    if M is not None:
        bits["edge_mask"] = O.constrained_edge_mask(inp["graph_matrix"], H).to(torch.uint8)
    return out, bits


def ref_model(R, name):
    """DCSVDTransformer(...).get_model() of lib/models/zinc/dc.py with the two cross-talk keys, MeanAbsoluteError; the way
    reference_cases.ref_model runs the shipped configurations"""
    inp, params, cfg = model_inputs(name)
    N = inp["graph_matrix"].shape[1]
    kw = dict(model_width=cfg["model_width"], edge_width=cfg["edge_width"], model_height=cfg["model_height"],
              upto_hop=cfg["upto_hop"], max_length=N, num_heads=H, use_svd=False, readout_edges=False,
              edge_channel_type=cfg["edge_channel_type"], num_virtual_nodes=0, distance_loss=0., node2edge_xtalk=cfg["node2edge_xtalk"],
              edge2node_xtalk=cfg["edge2node_xtalk"])
    feed = dict(node_features=inp["node_features"], feature_matrix=inp["feature_matrix"], graph_matrix=inp["graph_matrix"])
    state = {}

    def run(weights):
        m = R.zinc.DCSVDTransformer(**kw)
        with RX.session(feed=feed, weights=weights):
            state["y"] = m.get_model().outputs
        return m.tracked_layers

    tracked = run(RC._weights_for(run, params))
    y = state["y"]
    loss = R.tf.keras.losses.MeanAbsoluteError(name="MAE")(inp["target"], y)
    out = dict(y=y, loss=loss.reshape(1))
    L = tracked.get_layers_dict()
    bits = dict(node_mask=L["node_emb"].output._keras_mask.as_subclass(torch.Tensor))
    if cfg["edge_channel_type"] == "constrained":
        bits["edge_mask"] = L["adj_expand_mask"].output.as_subclass(torch.Tensor).to(torch.uint8)
    out.update({f"d/{k}": g for k, g in RC._grads_by_oracle_key(tracked, loss, params).items()})
    return dict(inputs=inp, weights=params, out=out, bits=bits)


def packed_ref_model(R, name):
    return RC.pack(ref_model(R, name), MODEL_CAP)


def fixture_path(name):
    return os.path.join(XT_DIR, f"{name}.npz")


def load(name):
    """the fixture in the form reference_cases.load returns"""
    z = np.load(fixture_path(name))
    fix = {k: z[k] for k in z.files if k.startswith("out/")}
    fix["sha"] = dict(zip(z["sha_names"].tolist(), z["sha"]))
    fix["stat"] = dict(zip(z["stat_names"].tolist(), z["stat"]))
    return fix
