"""The cases of tests/golden/scale_degree/: what the REFERENCE'S OWN model code computes with scale_degree, run unmodified on the
eager stand-in (oracle/ref_exec.py) in fp64, and what the oracle computes for the same inputs.

Shared by tests/golden/make_scale_degree_golden.py (writes the fixtures), tests/test_scale_degree_cpu.py (oracle against fixtures) and
tests/test_scale_degree_gpu.py (kernels against fixtures).  Also the shapes and input recipes of the GPU parity tests (SHAPES, make_case,
oracle), which the CPU file holds to their fairness bounds.  `ref_*` need the reference modules R of `ref_exec.reference()`; the
`*_inputs` recipes and `oracle_*` need nothing but this repository.

Fixture format (one .npz per file, whole tensors): inputs/<name>, weights/<oracle key> as the fp32 / integer arrays the seeded recipe
produces, out/<name> in fp64 (h_out, e_out, dh, de or y, loss; d/<oracle key> = the weight gradients).  The model case is two
files -- `model_zinc.npz` (inputs, weights, prediction, loss) and `model_zinc_grads.npz` (every weight gradient) -- to keep each under
the size limit of a committed file."""
from __future__ import annotations

import os

import numpy as np
import torch

import cases as CS
import reference_cases as RC
from oracle import egt_model_oracle as MO, egt_oracle as O, ref_exec as RX

DIR = os.path.join(CS.GOLDEN_DIR, "scale_degree")
MAX_BYTES = 650 * 1000
F64 = torch.float64
H = 8
SCALERS = ("log", "linear")
BLOCK_SHAPE = dict(B=2, N=19, Dh=64, De=16, nodes=[19, 13])          # one padded graph
MODEL_CFG = dict(model_width=64, edge_width=16, model_height=2, upto_hop=4, scale_degree=True, scaler_type="log")
MODEL_B, MODEL_N = 3, 19


# ------------------------------------------------------------------------------------ the GPU parity recipes -----
# (B, N, d, De, real nodes per graph, forward kernel, backward kernel) -- the plan without switches
SHAPES = {
    "n16_de64": (2, 16, 8, 64, [16, 16], "k_block_fwd/", "k_block_bwd_v5"),             # full N
    "n19_de64": (3, 19, 8, 64, [19, 11, 19], "k_block_fwd/", "k_block_bwd_v5"),         # ragged, one graph padded to 11
    "n37_d6_de48": (2, 37, 6, 48, [37, 30], "k_block_fwd/", "k_block_bwd_v5"),
    "n69_de64": (2, 69, 8, 64, [69, 60], "k_block_fwd/", "k_block_bwd_v5"),             # five key tiles: a wave owns two
    "n80_de16": (2, 80, 8, 16, [80, 71], "k_block_fwd_r4/", "k_block_bwd_v4r"),
    "n69_de8": (2, 69, 8, 8, [69, 60], "k_block_fwd_r4/", "k_block_bwd_v4r"),           # De = 8 on r4 / v4r
    "n150_d4_de8": (2, 150, 4, 8, [150, 131], "k_block_fwd_r4/8w", "k_block_bwd_v4r"),
}


def make_case(B, N, d, De, nodes, seed_name, ect="residual", gate_bias0=None, rand_p=None):
    """inputs, oracle parameters and attributes of one block (cases.make_block_case's recipe at the shape asked for)"""
    c = dict(B=B, N=N, Dh=8 * d, De=De, nodes=nodes, ect=ect)
    if rand_p:
        c["rand_p"] = rand_p
    inp, params, attrs, c = CS.make_block_case(seed_name, case=c)
    if gate_bias0 is not None:      # the "small degree" recipe: head 0's gates all but closed
        params["attention_gates.bias"] = params["attention_gates.bias"].clone()
        params["attention_gates.bias"][0] = gate_bias0
    return inp, params, attrs, c


def oracle(inp, params, attrs, scaler, rand_mask=None):
    used = {k: v for k, v in params.items() if attrs["edge_channel_type"] != "bias" or k.split(".")[0] not in ("norm_edge", "dense_edge_r")}
    return CS.block_oracle(dict(inp, rand_mask=rand_mask), used, dict(attrs, scale_degree=True, scaler_type=scaler))


# ------------------------------------------------------------------------------------------------------ block -----
def block_inputs(scaler):
    inp, params, attrs, _ = CS.make_block_case(f"scale_degree_{scaler}", case=BLOCK_SHAPE)
    return inp, params, dict(attrs, scale_degree=True, scaler_type=scaler)


def ref_block(R, scaler):
    """GraphTransformerBase.transform_embeddings with one layer and scale_degree (RC.ref_block's way: identity FFNs behind the block)"""
    inp, params, attrs = block_inputs(scaler)
    Dh, De = BLOCK_SHAPE["Dh"], BLOCK_SHAPE["De"]
    allp = {f"layer0.{k}": v for k, v in params.items()}
    allp.update(RC._filler_ffn("layer0.ffn_node", Dh))
    allp.update(RC._filler_ffn("layer0.ffn_edge", De))
    state = {}

    def run(weights):
        m = R.xformer_base.GraphTransformerBase(model_width=Dh, edge_width=De, num_heads=H, model_height=1, gate_attention=True,
                                                edge_channel_type="residual", scale_degree=True, scaler_type=scaler,
                                                do_final_norm=False, activation="elu")
        with RX.session(weights=weights):
            h = RX.wrap(inp["h"].double()).requires_grad_(); e = RX.wrap(inp["e"].double()).requires_grad_()
            h._keras_mask = RX.wrap(inp["mask"])
            m.transform_embeddings(h, e, None)
            state.update(h=h, e=e)
        return m.tracked_layers

    tracked = run(RC._weights_for(run, allp))
    L = tracked.get_layers_dict()
    h2, e2 = L["res_mha_00"].output, L["res_edge_00"].output
    loss = (h2 * inp["dh"].double()).sum() + (e2 * inp["de"].double()).sum()
    gh, ge = torch.autograd.grad(loss, [state["h"], state["e"]], retain_graph=True)
    out = dict(h_out=h2, e_out=e2, dh=gh, de=ge)
    gr = RX.weight_grads(tracked, loss)
    out.update({f"d/{k}": gr[RC.keras_name(f"layer0.{k}")] for k in params})
    return dict(inputs={k: v for k, v in inp.items() if v is not None}, weights=params, out=out)


def oracle_block(scaler):
    inp, params, attrs = block_inputs(scaler)
    r = CS.block_oracle(inp, params, attrs)
    out = {k: r[k] for k in ("h_out", "e_out", "dh", "de")}
    out.update({f"d/{k}": g for k, g in r["dparams"].items()})
    return out


# ------------------------------------------------------------------------------------------------------ model -----
def model_inputs():
    g = torch.Generator().manual_seed(1905)
    B, N = MODEL_B, MODEL_N
    n = torch.tensor([N, 12, 16])
    real = torch.arange(N)[None, :] < n[:, None]
    nf = torch.randint(0, 28, (B, N), generator=g)
    nf[~real] = -1
    adj = (torch.rand(B, N, N, generator=g) > 0.7).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (real[:, :, None] & real[:, None, :]).float()
    adj = adj * (1 - torch.eye(N))[None]
    fm = torch.where(adj > 0, torch.randint(0, 4, (B, N, N), generator=g), torch.tensor(-1))
    y = torch.randn(B, 1, generator=g)
    cfg = {k: v for k, v in MODEL_CFG.items() if k not in ("scale_degree", "scaler_type")}
    params = MO.init_zinc_params(cfg, dtype=torch.float32, generator=g)
    return dict(node_features=nf, feature_matrix=fm, graph_matrix=adj, target=y), params, dict(MODEL_CFG)


def ref_model(R):
    """DCSVDTransformer(scale_degree=True).get_model() of lib/models/zinc/dc.py and the scheme's MeanAbsoluteError"""
    inp, params, cfg = model_inputs()
    kw = dict(model_width=cfg["model_width"], edge_width=cfg["edge_width"], model_height=cfg["model_height"], upto_hop=cfg["upto_hop"],
              max_length=MODEL_N, num_heads=H, use_svd=False, readout_edges=False, num_virtual_nodes=0, scale_degree=True, scaler_type=cfg["scaler_type"])
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
    out.update({f"d/{k}": g for k, g in RC._grads_by_oracle_key(tracked, loss, params).items()})
    return dict(inputs=inp, weights=params, out=out)


def zinc_forward(nf, fm, adj, p, cfg):
    """egt_model_oracle.zinc_forward with the degree scalers handed to every block"""
    act = cfg.get("activation", "elu")
    h, e, mask = MO.zinc_embeddings(nf, fm, adj, p, cfg, None)
    for ii in range(cfg["model_height"]):
        bp = {k[len(f"layer{ii}."):]: v for k, v in p.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
        h, e = O.block_forward(h, e, mask, bp, num_heads=H, scale_degree=True, scaler_type=cfg["scaler_type"])
        e = O.ffn_forward(e, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_edge.")}, activation=act)
        h = O.ffn_forward(h, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_node.")}, activation=act)
    h = O.layer_norm(h, p["node_norm_final.gamma"], p["node_norm_final.beta"])
    x = MO.masked_global_avg_pool_1d(h, mask)
    x = MO.mlp_out(x, p, 2, act)
    return O.dense(x, p["target.kernel"], p["target.bias"])


def oracle_model():
    inp, params, cfg = model_inputs()
    p = {k: t.to(F64).requires_grad_() for k, t in params.items()}
    y = zinc_forward(inp["node_features"], inp["feature_matrix"], inp["graph_matrix"], p, cfg)
    loss = MO.mae_loss(y, inp["target"].to(F64))
    gr = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    out = dict(y=y.detach(), loss=loss.detach().reshape(1))
    out.update({f"d/{k}": (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(p, gr)})
    return out


# ---------------------------------------------------------------------------------------------------- fixtures -----
def _np(t, f64=False):
    a = t.detach().as_subclass(torch.Tensor)
    return (a.to(F64) if f64 else a).cpu().numpy()


def flat(case, groups=("inputs", "weights", "out"), out_filter=None):
    d = {}
    for grp in groups:
        for k, v in case[grp].items():
            if v is None or (grp == "out" and out_filter is not None and not out_filter(k)):
                continue
            d[f"{grp}/{k}"] = _np(v, f64=(grp == "out"))
    return d


def files(R):
    """{file name: flat dict} of every fixture"""
    out = {f"block_{s}.npz": flat(ref_block(R, s)) for s in SCALERS}
    m = ref_model(R)
    out["model_zinc.npz"] = flat(m, out_filter=lambda k: not k.startswith("d/"))
    out["model_zinc_grads.npz"] = flat(m, groups=("out",), out_filter=lambda k: k.startswith("d/"))
    return out


def load(name):
    z = np.load(os.path.join(DIR, name))
    return {k: z[k] for k in z.files}


def load_out(*names):
    """out/<k> of the named files as fp64 tensors"""
    return {k[4:]: torch.from_numpy(v) for n in names for k, v in load(n).items() if k.startswith("out/")}
