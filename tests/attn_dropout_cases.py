"""Attention dropout on the fused block (EGT_BF_ATTN_DROPOUT, EGTBlock(fused_attn_dropout=True)): the shape table and input recipes
of the GPU parity tests, and the cases of tests/golden/attn_dropout/ -- what the REFERENCE'S OWN model code computes with
attn_dropout, run unmodified on the eager stand-in (oracle/ref_exec.py) in fp64 with the keep masks of the kernels' counter stream
injected (oracle/rng_ref.py: dropout_keep), and what the oracle computes for the same inputs.

Shared by tests/golden/make_attn_dropout_golden.py (writes the fixtures), tests/test_attn_dropout_cpu.py (plan, oracle against fixtures)
and tests/test_attn_dropout_gpu.py (kernels against oracle and fixtures).  `ref_*` need the reference modules R of
`ref_exec.reference()`; everything else needs nothing but this repository.

Fixture format: as tests/golden/scale_degree/ (inputs/<name>, weights/<oracle key> as the seeded recipe's fp32 / integer arrays,
out/<name> in fp64).  The keep masks are not stored: they are a function of the seed (rng_ref), which the fixtures' cases fix."""
from __future__ import annotations

import os

import numpy as np
import torch

import cases as CS
import reference_cases as RC
from oracle import egt_model_oracle as MO, egt_oracle as O, ref_exec as RX, rng_ref

DIR = os.path.join(CS.GOLDEN_DIR, "attn_dropout")
MAX_BYTES = 650 * 1000
F64 = torch.float64
H = 8
GOLD, STEP, M64 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xFFFFFFFFFFFFFFFF
# the two recipes of every parity row: the rate alone; the rate together with the in-kernel random mask
RATES = {"p25": (0.25, 0.0), "p10_rm10": (0.1, 0.1)}

# (B, N, d, De, real nodes per graph, forward kernel, backward kernel) -- the plan of the flagged descriptor without switches.
# fp32 edge tensors; De = 8 runs on r4 / v4r (the De = 8 VALU kernels draw no dropout)
SHAPES = {
    "n16_de64": (2, 16, 8, 64, [16, 16], "k_block_fwd/", "k_block_bwd_v5"),             # full N
    "n19_de64": (3, 19, 8, 64, [19, 11, 19], "k_block_fwd/", "k_block_bwd_v5"),         # ragged, one graph padded to 11
    "n37_d6_de48": (2, 37, 6, 48, [37, 30], "k_block_fwd/", "k_block_bwd_v5"),
    "n69_de64": (2, 69, 8, 64, [69, 60], "k_block_fwd/", "k_block_bwd_v5"),             # five key tiles: a wave owns two
    "n80_de16": (2, 80, 8, 16, [80, 71], "k_block_fwd_r4/", "k_block_bwd_v4r"),
    "n69_de8": (2, 69, 8, 8, [69, 60], "k_block_fwd_r4/", "k_block_bwd_v4r"),           # De = 8 on r4 / v4r
    "n150_d4_de8": (2, 150, 4, 8, [150, 131], "k_block_fwd_r4/8w", "k_block_bwd_v4r"),  # eight-wave r4
}
# further rows: (shape, what differs) -> the families they reach
VARIANTS = {
    "constrained_n19_de64": dict(shape="n19_de64", ect="constrained", fwd="k_block_fwd/", bwd="k_block_bwd_v4"),
    "constrained_n37_d6_de48": dict(shape="n37_d6_de48", ect="constrained", fwd="k_block_fwd/", bwd="k_block_bwd_v4"),
    "ungated_n19_de64": dict(shape="n19_de64", gate=False, fwd="k_block_fwd/", bwd="k_block_bwd_v5"),
    "bias_n69_de8": dict(shape="n69_de8", ect="bias", fwd="k_block_fwd_r4/", bwd="k_block_bwd_v4r"),
    "bias_n19_de64": dict(shape="n19_de64", ect="bias", fwd="k_block_fwd/", bwd="k_block_bwd_v5"),
}
BF16_ROWS = {"n19_de64": ("k_block_fwd/", "k_block_bwd_v4"), "n69_de8": ("k_block_fwd_r4/", "k_block_bwd_v4r")}


def first_seed(module_seed: int, calls: int = 1) -> int:
    """what EGT.next_seed() returns on call number `calls` of a module constructed with `seed=module_seed`"""
    return (module_seed * GOLD + calls * STEP) & M64


def keep_of(seed, B, N, rate):
    """the keep mask [B, N, N, H] the kernels draw for a call that consumed `seed`"""
    return torch.from_numpy(rng_ref.dropout_keep(seed, B, N, H, rate))


def rand_of(seed, B, N, prob):
    return torch.from_numpy(rng_ref.random_mask(seed, B, N, H, prob)) if prob > 0 else None


def make_case(B, N, d, De, nodes, seed_name, ect="residual", gate=True, rand_p=None):
    """inputs, oracle parameters and attributes of one block (cases.make_block_case's recipe at the shape asked for)"""
    c = dict(B=B, N=N, Dh=8 * d, De=De, nodes=nodes, ect=ect, gate=gate)
    if rand_p:
        c["rand_p"] = rand_p
    return CS.make_block_case(seed_name, case=c)


def make_row(name, seed_suffix=""):
    """the case of a SHAPES or VARIANTS row: (inp, params, attrs, c, forward family, backward family)"""
    v = VARIANTS.get(name, dict(shape=name))
    B, N, d, De, nodes, ffwd, fbwd = SHAPES[v["shape"]]
    inp, params, attrs, c = make_case(B, N, d, De, nodes, name + seed_suffix, ect=v.get("ect", "residual"), gate=v.get("gate", True))
    return inp, params, attrs, c, v.get("fwd", ffwd), v.get("bwd", fbwd)


def oracle(inp, params, attrs, rate, keep, rand_mask=None):
    """the fp64 block with the injected samples: `attrs` carries drop_keep / attn_dropout straight into O.block_forward"""
    ect = attrs["edge_channel_type"]
    used = {k: v for k, v in params.items()
            if (ect != "bias" or k.split(".")[0] not in ("norm_edge", "dense_edge_r")) and (attrs["gate_attention"] or not k.startswith("attention_gates"))}
    return CS.block_oracle(dict(inp, rand_mask=rand_mask), used, dict(attrs, drop_keep=keep, attn_dropout=rate))


# ------------------------------------------------------------------------------------------------------ block -----
BLOCK_SHAPE = dict(B=2, N=19, Dh=64, De=16, nodes=[19, 13])          # one padded graph
BLOCK_SEED = 11                                                       # EGTBlock(seed=BLOCK_SEED): the first call's seed is first_seed(11)
BLOCK_FIXTURES = {"block_p25": "p25", "block_p10_rm10": "p10_rm10"}


def block_inputs(fix):
    rate, prob = RATES[BLOCK_FIXTURES[fix]]
    inp, params, attrs, _ = CS.make_block_case(f"attn_dropout_{fix}", case=BLOCK_SHAPE)
    seed = first_seed(BLOCK_SEED)
    B, N = BLOCK_SHAPE["B"], BLOCK_SHAPE["N"]
    inp = dict(inp, rand_mask=rand_of(seed, B, N, prob))
    return inp, params, dict(attrs, attn_dropout=rate, drop_keep=keep_of(seed, B, N, rate)), prob


def ref_block(R, fix):
    """GraphTransformerBase.transform_embeddings with one layer and attn_dropout (RC.ref_block's way: identity FFNs behind the block),
    in training mode with the keep mask -- and the random mask -- of the kernels' streams injected"""
    inp, params, attrs, prob = block_inputs(fix)
    Dh, De = BLOCK_SHAPE["Dh"], BLOCK_SHAPE["De"]
    allp = {f"layer0.{k}": v for k, v in params.items()}
    allp.update(RC._filler_ffn("layer0.ffn_node", Dh))
    allp.update(RC._filler_ffn("layer0.ffn_edge", De))
    state = {}

    def run(weights):
        m = R.xformer_base.GraphTransformerBase(model_width=Dh, edge_width=De, num_heads=H, model_height=1, gate_attention=True,
                                                edge_channel_type="residual", attn_dropout=attrs["attn_dropout"], random_mask_prob=prob,
                                                do_final_norm=False, activation="elu")
        uniform = [] if inp["rand_mask"] is None else [torch.where(inp["rand_mask"], 0.0, 1.0)]
        with RX.session(training=True, uniform=uniform, keep=[attrs["drop_keep"].double()], weights=weights):
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


def oracle_block(fix):
    inp, params, attrs, _ = block_inputs(fix)
    r = CS.block_oracle(inp, params, attrs)
    out = {k: r[k] for k in ("h_out", "e_out", "dh", "de")}
    out.update({f"d/{k}": g for k, g in r["dparams"].items()})
    return out


# ------------------------------------------------------------------------------------------------------ model -----
MODEL_CFG = dict(model_width=64, edge_width=16, model_height=2, upto_hop=4, attn_dropout=0.1)
MODEL_B, MODEL_N = 3, 19


def model_seeds():
    """the seed layer i of ZincDCTransformer(seed=0) consumes on its first training call (EGTLayerStack: block seed = i)"""
    return [first_seed(i) for i in range(MODEL_CFG["model_height"])]


def model_keeps():
    return [keep_of(s, MODEL_B, MODEL_N, MODEL_CFG["attn_dropout"]) for s in model_seeds()]


def model_inputs():
    g = torch.Generator().manual_seed(2207)
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
    cfg = {k: v for k, v in MODEL_CFG.items() if k != "attn_dropout"}
    params = MO.init_zinc_params(cfg, dtype=torch.float32, generator=g)
    return dict(node_features=nf, feature_matrix=fm, graph_matrix=adj, target=y), params, dict(MODEL_CFG)


def ref_model(R):
    """DCSVDTransformer(attn_dropout=0.1, random_mask_prob=0).get_model() of lib/models/zinc/dc.py in training mode, the layers' keep
    masks injected in layer order, and the scheme's MeanAbsoluteError"""
    inp, params, cfg = model_inputs()
    kw = dict(model_width=cfg["model_width"], edge_width=cfg["edge_width"], model_height=cfg["model_height"], upto_hop=cfg["upto_hop"],
              max_length=MODEL_N, num_heads=H, use_svd=False, readout_edges=False, num_virtual_nodes=0, attn_dropout=cfg["attn_dropout"],
              random_mask_prob=0.0)
    feed = dict(node_features=inp["node_features"], feature_matrix=inp["feature_matrix"], graph_matrix=inp["graph_matrix"])
    state = {}

    def run(weights):
        m = R.zinc.DCSVDTransformer(**kw)
        with RX.session(training=True, feed=feed, keep=[k.double() for k in model_keeps()], weights=weights):
            state["y"] = m.get_model().outputs
        return m.tracked_layers

    tracked = run(RC._weights_for(run, params))
    y = state["y"]
    loss = R.tf.keras.losses.MeanAbsoluteError(name="MAE")(inp["target"], y)
    out = dict(y=y, loss=loss.reshape(1))
    out.update({f"d/{k}": g for k, g in RC._grads_by_oracle_key(tracked, loss, params).items()})
    return dict(inputs=inp, weights=params, out=out)


def zinc_forward(nf, fm, adj, p, cfg, keeps):
    """egt_model_oracle.zinc_forward with a keep mask handed to every block"""
    act = cfg.get("activation", "elu")
    h, e, mask = MO.zinc_embeddings(nf, fm, adj, p, cfg, None)
    for ii in range(cfg["model_height"]):
        bp = {k[len(f"layer{ii}."):]: v for k, v in p.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
        h, e = O.block_forward(h, e, mask, bp, num_heads=H, drop_keep=keeps[ii], attn_dropout=cfg["attn_dropout"])
        e = O.ffn_forward(e, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_edge.")}, activation=act)
        h = O.ffn_forward(h, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_node.")}, activation=act)
    h = O.layer_norm(h, p["node_norm_final.gamma"], p["node_norm_final.beta"])
    x = MO.masked_global_avg_pool_1d(h, mask)
    x = MO.mlp_out(x, p, 2, act)
    return O.dense(x, p["target.kernel"], p["target.bias"])


def oracle_model():
    inp, params, cfg = model_inputs()
    p = {k: t.to(F64).requires_grad_() for k, t in params.items()}
    y = zinc_forward(inp["node_features"], inp["feature_matrix"], inp["graph_matrix"], p, cfg, model_keeps())
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


FILES = sorted([f"{f}.npz" for f in BLOCK_FIXTURES] + ["model_zinc.npz", "model_zinc_grads.npz"])


def files(R):
    """{file name: flat dict} of every fixture"""
    out = {f"{f}.npz": flat(ref_block(R, f)) for f in BLOCK_FIXTURES}
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
