"""The cases of tests/golden/reference/: what the REFERENCE'S OWN model code computes, run unmodified on the eager stand-in
(oracle/ref_exec.py, oracle/tf_eager) in fp64, and what the oracle computes for the same inputs.

Shared by tests/golden/make_reference_golden.py (writes the fixtures), tests/test_reference_exec_cpu.py (regeneration, oracle
against reference) and tests/test_reference_golden_gpu.py (kernels against the reference's numbers).  `ref_case(R, family,
name)` needs the reference modules R of `ref_exec.reference()`; `oracle_case(family, name)` and the `*_inputs(name)` recipes
need nothing but this repository.

Fixture format (one .npz per case; the size limits rule out whole tensors -- a two-layer width-64 model alone has 1.2 MB of
fp64 gradients):
    sha_names, sha          SHA-256 over dtype, shape and bytes of: inputs/<name>, weights/<name> -- the fp32 / integer arrays the
                            seeded recipe produces -- and bits/<name> -- an integer / boolean OUTPUT (masks, distance target),
                            compared bit for bit
    out/<tensor>            fp64 values: the whole tensor up to the family's cap (512 elements for the block-level families,
                            128 for stacks and models), else that many elements at the flat indices sample_index(tensor, n, cap)
    stat_names, stat        [sum, sum of squares, max |x|] of every WHOLE fp64 tensor: both test files hold the whole tensors
                            of the code under test to them, so no element is outside every check
With the reference present the CPU tests also compare every whole tensor element by element.
"""
from __future__ import annotations

import hashlib
import os
import zlib

import numpy as np
import torch

import cases as CS
import distance_ref as DR
import egt_simple_ref as ES
import virtual_nodes_ref as VR
from oracle import egt_model_oracle as MO, egt_oracle as O, ref_exec as RX

REF_DIR = os.path.join(CS.GOLDEN_DIR, "reference")
CAP = {"attn": 512, "block": 512, "ffn": 512, "stack": 128, "model": 128}
H = 8
FFN_NAMES = CS.FFN_NAMES
F64 = torch.float64


# ------------------------------------------------------------------------------------------ fixture format -----
def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    h = hashlib.sha256()
    h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def sample_index(key, n, cap):
    """`cap` of the flat indices 0..n-1, from numpy's frozen legacy generator seeded by the tensor's name"""
    rs = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    return np.sort(rs.choice(n, cap, replace=False)).astype(np.int64)


def pack(case, cap):
    """{'inputs': {..}, 'weights': {..}, 'out': {..fp64..}, 'bits': {..int/bool..}} -> the flat dict that is saved"""
    flat, shas, stats = {}, {}, {}
    for grp in ("inputs", "weights"):
        for k, v in case[grp].items():
            if v is not None:
                shas[f"{grp}/{k}"] = sha(v)
    for k, v in case["bits"].items():
        shas[f"bits/{k}"] = sha(v)
    for k, v in case["out"].items():
        a = v.detach().as_subclass(torch.Tensor).to(F64).numpy().reshape(-1)
        stats[k] = [a.sum(), (a * a).sum(), np.abs(a).max() if a.size else 0.0]
        if a.size > cap:
            a = a[sample_index(k, a.size, cap)]
        flat[f"out/{k}"] = a.copy()
    flat["sha_names"], flat["sha"] = np.array(list(shas)), np.stack(list(shas.values()))
    flat["stat_names"], flat["stat"] = np.array(list(stats)), np.array(list(stats.values()), dtype=np.float64)
    return flat


def load(family, name):
    """-> the fixture: out/<k> arrays and the dicts 'sha' ({name: digest}) and 'stat' ({tensor: [sum, sumsq, max]})"""
    z = np.load(os.path.join(REF_DIR, f"{family}_{name}.npz"))
    fix = {k: z[k] for k in z.files if k.startswith("out/")}
    fix["sha"] = dict(zip(z["sha_names"].tolist(), z["sha"]))
    fix["stat"] = dict(zip(z["stat_names"].tolist(), z["stat"]))
    return fix


def picked(fix, key, tensor):
    """the elements of `tensor` that the fixture stores under out/<key>, as a flat fp64 tensor"""
    a = tensor.detach().as_subclass(torch.Tensor).double().cpu().reshape(-1)
    stored = fix[f"out/{key}"].size
    assert a.numel() >= stored, f"{key}: {a.numel()} elements against {stored} stored"
    if a.numel() > stored:
        a = a[torch.from_numpy(sample_index(key, a.numel(), stored))]
    return a


# ------------------------------------------------------------------------------------------------ names -----
def keras_name(k):
    """oracle parameter key -> `<Keras layer name>/<weight name>`"""
    parts = k.split(".")
    if parts[0].startswith("layer") and parts[0][5:].isdigit():
        tag = f"{int(parts[0][5:]):02d}"
        if parts[1].startswith("ffn_"):
            ch, (what, attr) = parts[1][4:], parts[2].split("_")
            if what == "norm":
                return f"norm_fnn_{ch}_{tag}/{attr}"
            return f"fnn_{what}_{ch}_{tag}/{attr}"
        return f"{parts[1]}_{tag}/{parts[2]}"
    assert len(parts) == 2, k
    return f"{parts[0]}/{parts[1]}"


def to_keras(params):
    return {keras_name(k): v for k, v in params.items()}


def _created(run):
    """the weight names a run of reference code creates (a first pass whose NaN weights are thrown away)"""
    return list(RX.named_weights(run(None)))


def _weights_for(run, params):
    kp = to_keras(params)
    names = _created(run)
    missing = [n for n in names if n not in kp]
    assert not missing, f"the reference creates weights the oracle's parameter set lacks: {missing}"
    extra = sorted(set(kp) - set(names))
    assert not extra, f"the oracle's parameter set has weights the reference never creates: {extra}"
    return {n: kp[n] for n in names}


def _grads_by_oracle_key(tracked, loss, params):
    g = RX.weight_grads(tracked, loss)
    return {k: g[keras_name(k)] for k in params}


def _filler_ffn(prefix, W, mult=2.0):
    """FFN weights for runs whose subject is the attention block: lr2 = 0 makes the ffn_block the identity, bit for bit"""
    hid = round(W * mult)
    return {f"{prefix}.norm_gamma": torch.ones(W), f"{prefix}.norm_beta": torch.zeros(W),
            f"{prefix}.lr1_kernel": torch.full((W, hid), 0.01), f"{prefix}.lr1_bias": torch.zeros(hid),
            f"{prefix}.lr2_kernel": torch.zeros(hid, W), f"{prefix}.lr2_bias": torch.zeros(W)}


# ------------------------------------------------------------------------------------------- inner op -----
# beside cases.ATTN_CASES: d = 16 at eight heads, the geometry the MFMA inner op covers (its only d = 16 case has four heads)
EXTRA_ATTN_CASES = {"mfma_d16_n37": dict(B=2, N=37, H=8, d=16, nodes=[37, 30])}
ATTN_NAMES = list(CS.ATTN_CASES) + list(EXTRA_ATTN_CASES)


def make_attn_case(name):
    return CS.make_attn_case(name, case=EXTRA_ATTN_CASES.get(name))


def attn_inputs(name):
    inp, attrs, c = make_attn_case(name)
    return inp, {}, (attrs, c)


def ref_attn(R, name):
    inp, _, (attrs, c) = attn_inputs(name)
    layer = R.egt_layers.EGT(edge_input=inp["E"] is not None, gate_input=inp["G"] is not None, attn_mask=inp["M"] is not None,
                             random_mask_prob=c.get("rand_p", 0.0), name="mha", **attrs)
    uniform = [] if inp["rand_mask"] is None else [torch.where(inp["rand_mask"], 0.0, 1.0)]      # u < p exactly where masked
    keep = [] if inp["drop_keep"] is None else [inp["drop_keep"]]
    with RX.session(training=bool(uniform or keep), uniform=uniform, keep=keep):
        lv = lambda t: None if t is None else RX.wrap(t.double()).requires_grad_()
        QKV, E, G = lv(inp["QKV"]), lv(inp["E"]), lv(inp["G"])
        QKV._keras_mask = None if inp["mask"] is None else RX.wrap(inp["mask"])
        args = [QKV] + [t for t in (E, G) if t is not None] + ([] if inp["M"] is None else [RX.wrap(inp["M"].double())])
        V, Hh, At = layer(args)
        wrt = [t for t in (QKV, E, G) if t is not None]
        gr = iter(torch.autograd.grad((V * inp["dV"].double()).sum() + (Hh * inp["dH"].double()).sum(), wrt))
    out = dict(V_att=V, H_hat=Hh, A_tild=At, dQKV=next(gr))
    if E is not None:
        out["dE"] = next(gr)
    if G is not None:
        out["dG"] = next(gr)
    return dict(inputs=inp, weights={}, out=out, bits={})


def oracle_attn(name):
    inp, _, (attrs, _) = attn_inputs(name)
    return {k: v for k, v in CS.attn_oracle(inp, attrs).items() if v is not None}, {}


# ---------------------------------------------------------------------------- block (edge_update_* + mha_block) -----
VARIANT_SHAPE = dict(add_n_norm=(2, 19, 64, 32, 31), dropout=(2, 17, 64, 16, 47))      # tests/test_block_variants_gpu.py
BLOCK_VARIANTS = {f"addnorm_{ect}_{'gated' if gate else 'ungated'}": dict(kind="add_n_norm", ect=ect, gate=gate)
                  for ect, gate in [("residual", True), ("residual", False), ("none", True), ("bias", True)]}
BLOCK_VARIANTS.update({f"dropout_n{int(pn * 100)}_e{int(pe * 100)}": dict(kind="dropout", pn=pn, pe=pe)
                       for pn, pe in [(0.3, 0.0), (0.0, 0.25), (0.2, 0.4)]})
BLOCK_NAMES = list(CS.BLOCK_CASES) + list(BLOCK_VARIANTS)


def variant_inputs(name):
    """the inputs of tests/test_block_variants_gpu.py (_mk and the keep masks drawn after it)"""
    v = BLOCK_VARIANTS[name]
    B, N, Dh, De, seed = VARIANT_SHAPE[v["kind"]]
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, N, Dh, generator=g); e = torch.randn(B, N, N, De, generator=g) * 1.2
    dh = torch.randn(B, N, Dh, generator=g); de = torch.randn(B, N, N, De, generator=g)
    mask = torch.ones(B, N, dtype=torch.bool); mask[B - 1, N - 3:] = False
    params = O.init_block_params(Dh, De, 8, generator=g, randomize_norm=True)
    inp = dict(h=h, e=e, dh=dh, de=de, mask=mask, attn_mask=None, rand_mask=None, node_keep=None, edge_keep=None)
    attrs = dict(num_heads=H, edge_channel_type=v.get("ect", "residual"), gate_attention=v.get("gate", True), edge_activation=None)
    if v["kind"] == "add_n_norm":
        attrs["add_n_norm"] = True
    else:
        inp["node_keep"] = torch.rand(h.shape, generator=g) >= v["pn"]
        inp["edge_keep"] = torch.rand(e.shape, generator=g) >= v["pe"]
        attrs.update(node_dropout=v["pn"], edge_dropout=v["pe"])
    return inp, params, attrs


def block_inputs(name):
    if name in BLOCK_VARIANTS:
        return variant_inputs(name)
    inp, params, attrs, _ = CS.make_block_case(name)
    return dict(inp, node_keep=None, edge_keep=None), params, attrs


def _used_block_params(params, attrs):
    ect, gate = attrs["edge_channel_type"], attrs["gate_attention"]
    drop = set()
    if ect in ("bias", "none"):
        drop |= {"norm_edge", "dense_edge_r"}
    if ect == "none":
        drop |= {"attention_gates", "dense_edge_b"}
    if not gate:
        drop |= {"attention_gates"}
    return {k: v for k, v in params.items() if k.split(".")[0] not in drop}


def _base(R, Dh, De, attrs, height=1, final_norm=False, rand_p=0.0, activation="elu"):
    return R.xformer_base.GraphTransformerBase(
        model_width=Dh, edge_width=De, num_heads=H, model_height=height, gate_attention=attrs.get("gate_attention", True),
        edge_channel_type=attrs.get("edge_channel_type", "residual"), edge_activation=attrs.get("edge_activation"),
        add_n_norm=attrs.get("add_n_norm", False), node_dropout=attrs.get("node_dropout", 0.0),
        edge_dropout=attrs.get("edge_dropout", 0.0), random_mask_prob=rand_p, do_final_norm=final_norm, activation=activation)


def ref_block(R, name):
    """GraphTransformerBase.transform_embeddings with one layer: h', e' are what the attention part hands to the ffn_block
    (the outputs of res_mha_00 / res_edge_00, or of the norms behind them with add_n_norm)"""
    inp, params, attrs = block_inputs(name)
    Dh, De = inp["h"].shape[-1], inp["e"].shape[-1]
    ect = attrs["edge_channel_type"]
    used = _used_block_params(params, attrs)
    allp = {f"layer0.{k}": v for k, v in used.items()}
    allp.update(_filler_ffn("layer0.ffn_node", Dh))
    if ect in ("residual", "constrained"):
        allp.update(_filler_ffn("layer0.ffn_edge", De))
    rand_p = 0.25 if inp["rand_mask"] is not None else 0.0
    training = inp["rand_mask"] is not None or inp["node_keep"] is not None
    state = {}

    def run(weights):
        m = _base(R, Dh, De, attrs, rand_p=rand_p)
        uniform = [] if inp["rand_mask"] is None else [torch.where(inp["rand_mask"], 0.0, 1.0)]
        kbn = {}
        if attrs.get("node_dropout", 0) > 0:
            kbn.update(drp_mha_00=inp["node_keep"], drp_fnn_node_00=torch.ones_like(inp["h"]))
        if attrs.get("edge_dropout", 0) > 0:
            kbn.update(drp_edge_00=inp["edge_keep"], drp_fnn_edge_00=torch.ones_like(inp["e"]))
        with RX.session(training=training, uniform=uniform, keep_by_name=kbn, weights=weights):
            h = RX.wrap(inp["h"].double()).requires_grad_(); e = RX.wrap(inp["e"].double()).requires_grad_()
            h._keras_mask = RX.wrap(inp["mask"])
            M = None if inp["attn_mask"] is None else RX.wrap(inp["attn_mask"].double())
            m.transform_embeddings(h, e, M)
            state.update(h=h, e=e)
        return m.tracked_layers

    tracked = run(_weights_for(run, allp))
    L = tracked.get_layers_dict()
    post = attrs.get("add_n_norm", False)
    h2 = L["norm_mha_00" if post else "res_mha_00"].output
    e2 = L["norm_edge_00" if post else "res_edge_00"].output if ect in ("residual", "constrained") else state["e"]
    loss = (h2 * inp["dh"].double()).sum() + (e2 * inp["de"].double()).sum()
    gh, ge = torch.autograd.grad(loss, [state["h"], state["e"]], retain_graph=True, allow_unused=True)
    out = dict(h_out=h2, e_out=e2, dh=gh, de=ge if ge is not None else torch.zeros_like(state["e"]))
    gr = RX.weight_grads(tracked, loss)
    out.update({f"d/{k}": gr[keras_name(f"layer0.{k}")] for k in used})
    return dict(inputs={k: v for k, v in inp.items() if v is not None}, weights=params, out=out, bits={})


def oracle_block(name):
    inp, params, attrs = block_inputs(name)
    cv = lambda t: None if t is None else t.to(F64)
    h = cv(inp["h"]).requires_grad_(); e = cv(inp["e"]).requires_grad_()
    used = _used_block_params(params, attrs)
    p = {k: v.to(F64).requires_grad_() for k, v in used.items()}
    h2, e2 = O.block_forward(h, e, inp["mask"], p, attn_mask=cv(inp["attn_mask"]), rand_mask=inp["rand_mask"],
                             node_keep=inp["node_keep"], edge_keep=inp["edge_keep"], **attrs)
    loss = (h2 * cv(inp["dh"])).sum() + (e2 * cv(inp["de"])).sum()
    gr = torch.autograd.grad(loss, [h, e] + list(p.values()), allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=gr[0], de=z(gr[1], e))
    out.update({f"d/{k}": z(g, p[k]) for k, g in zip(p, gr[2:])})
    return out, {}


# --------------------------------------------------------------------------------------------- ffn_block -----
def ffn_inputs(name):
    inp, params, c = CS.make_ffn_case(name)
    return inp, params, c


def ref_ffn(R, name):
    """the ffn_block of one layer of transform_embeddings, with the attention part in front of it made the identity
    (dense_mha and dense_edge_r all zero: h' = 0 + h, e' = 0 + e bit for bit)"""
    inp, params, c = ffn_inputs(name)
    x, W = inp["x"], c["W"]
    edge = x.dim() == 4
    B, N = x.shape[0], x.shape[1]
    Dh, De = (64, W) if edge else (W, 8)
    g = torch.Generator().manual_seed(5)
    other = torch.randn(B, N, Dh, generator=g) if edge else torch.randn(B, N, N, De, generator=g)
    blk = O.init_block_params(Dh, De, H, generator=g, randomize_norm=True)
    for k in ("dense_mha.kernel", "dense_mha.bias", "dense_edge_r.kernel", "dense_edge_r.bias"):
        blk[k] = torch.zeros_like(blk[k])
    allp = {f"layer0.{k}": v for k, v in blk.items()}
    mine, filler = ("edge", "node") if edge else ("node", "edge")
    allp.update({f"layer0.ffn_{mine}.{k}": v for k, v in params.items()})
    allp.update(_filler_ffn(f"layer0.ffn_{filler}", Dh if edge else De))
    state = {}

    def run(weights):
        m = _base(R, Dh, De, {}, activation=c["act"])
        with RX.session(weights=weights):
            xx = RX.wrap(x.double()).requires_grad_()
            h, e = (RX.wrap(other.double()), xx) if edge else (xx, RX.wrap(other.double()))
            h._keras_mask = RX.wrap(torch.ones(B, N, dtype=torch.bool))
            m.transform_embeddings(h, e, None)
            state["x"] = xx
        return m.tracked_layers

    tracked = run(_weights_for(run, allp))
    L = tracked.get_layers_dict()
    fed = L[f"res_{'edge' if edge else 'mha'}_00"].output
    assert torch.equal(fed, state["x"]), "the attention part in front of the FFN is not the identity"
    y = L[f"res_fnn_{mine}_00"].output
    loss = (y * inp["dy"].double()).sum()
    out = dict(y=y, dx=torch.autograd.grad(loss, state["x"], retain_graph=True)[0])
    gr = RX.weight_grads(tracked, loss)
    out.update({f"d/{k}": gr[keras_name(f"layer0.ffn_{mine}.{k}")] for k in FFN_NAMES})
    return dict(inputs=inp, weights=params, out=out, bits={})


def oracle_ffn(name):
    inp, params, c = ffn_inputs(name)
    r = CS.ffn_oracle(inp, params, c)
    out = dict(y=r["y"], dx=r["dx"])
    out.update({f"d/{k}": v for k, v in r["dparams"].items()})
    return out, {}


# ------------------------------------------------------------------------------------------------- stack -----
STACK_CASES = {"n23_de8": dict(N=23, De=8), "n32_de64": dict(N=32, De=64)}


def stack_inputs(name):
    """two layers with both FFNs and the final norms; the inputs of test_layer_stack_attention_plus_ffn_vs_oracle"""
    c = STACK_CASES[name]
    N, De, B, Dh, Ly = c["N"], c["De"], 2, 64, 2
    g = torch.Generator().manual_seed(2)
    h = torch.randn(B, N, Dh, generator=g); e = torch.randn(B, N, N, De, generator=g)
    mask = torch.ones(B, N, dtype=torch.bool); mask[0, N - 4:] = False
    dh = torch.randn(B, N, Dh, generator=g); de = torch.randn(B, N, N, De, generator=g)
    cfg = dict(model_width=Dh, edge_width=De, model_height=Ly, upto_hop=1)
    full = MO.init_zinc_params(cfg, dtype=torch.float32, generator=g)
    params = {k: v for k, v in full.items() if k.startswith("layer") or "norm_final" in k}
    return dict(h=h, e=e, mask=mask, dh=dh, de=de), params, cfg


def ref_stack(R, name):
    inp, params, cfg = stack_inputs(name)
    state = {}

    def run(weights):
        m = _base(R, cfg["model_width"], cfg["edge_width"], {}, height=cfg["model_height"], final_norm=True)
        with RX.session(weights=weights):
            h = RX.wrap(inp["h"].double()).requires_grad_(); e = RX.wrap(inp["e"].double()).requires_grad_()
            h._keras_mask = RX.wrap(inp["mask"])
            h2, e2 = m.transform_embeddings(h, e, None)
            state.update(h=h, e=e, h2=h2, e2=e2)
        return m.tracked_layers

    tracked = run(_weights_for(run, params))
    loss = (state["h2"] * inp["dh"].double()).sum() + (state["e2"] * inp["de"].double()).sum()
    gh, ge = torch.autograd.grad(loss, [state["h"], state["e"]], retain_graph=True)
    out = dict(h_out=state["h2"], e_out=state["e2"], dh=gh, de=ge)
    out.update({f"d/{k}": v for k, v in _grads_by_oracle_key(tracked, loss, params).items()})
    return dict(inputs=inp, weights=params, out=out, bits={})


def _layer_loop(h, e, mask, p, Ly, attn_mask=None, act="elu"):
    for ii in range(Ly):
        bp = {k[len(f"layer{ii}."):]: v for k, v in p.items() if k.startswith(f"layer{ii}.") and ".ffn_" not in k}
        h, e = O.block_forward(h, e, mask, bp, num_heads=H, attn_mask=attn_mask)
        e = O.ffn_forward(e, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_edge.")}, activation=act)
        h = O.ffn_forward(h, {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith(f"layer{ii}.ffn_node.")}, activation=act)
    return h, e


def oracle_stack(name):
    inp, params, cfg = stack_inputs(name)
    p = {k: v.to(F64).requires_grad_() for k, v in params.items()}
    h = inp["h"].double().requires_grad_(); e = inp["e"].double().requires_grad_()
    h2, e2 = _layer_loop(h, e, inp["mask"], p, cfg["model_height"])
    h2 = O.layer_norm(h2, p["node_norm_final.gamma"], p["node_norm_final.beta"])
    e2 = O.layer_norm(e2, p["edge_norm_final.gamma"], p["edge_norm_final.beta"])
    loss = (h2 * inp["dh"].double()).sum() + (e2 * inp["de"].double()).sum()
    gr = torch.autograd.grad(loss, [h, e] + list(p.values()))
    out = dict(h_out=h2.detach(), e_out=e2.detach(), dh=gr[0], de=gr[1])
    out.update({f"d/{k}": g for k, g in zip(p, gr[2:])})
    return out, {}


# ------------------------------------------------------------------------------------------------ models -----
DIST_W, DIST_T = 0.05, 8
MODEL_VARIANTS = {"plain": {}, "nv1": dict(num_virtual_nodes=1), "nv2": dict(num_virtual_nodes=2),
                  "dist": dict(distance_loss=DIST_W, distance_target=DIST_T),
                  "constrained": dict(edge_channel_type="constrained"), "bias": dict(edge_channel_type="bias")}
MODEL_NAMES = [f"{c}_{v}" for c in CS.MODEL_CASES for v in MODEL_VARIANTS] + ["cifar10_n21_de8"]
CIFAR_CFG = dict(model_width=64, edge_width=8, model_height=2, upto_hop=4, num_targets=10)


def model_inputs(name):
    """-> (kind, inputs, fp32 parameters under the oracle's keys, model config, variant keys)"""
    if name == "cifar10_n21_de8":
        g = torch.Generator().manual_seed(2121)
        inp = VR.graphs("cifar10", 2, 21, [21, 13], g)
        p = MO.init_zinc_params(dict(CIFAR_CFG, float_node_features=5, float_edge_features=1), dtype=torch.float32, generator=g)
        p.pop("node_emb.embeddings"); p.pop("fm_emb.embeddings")
        return "cifar10", inp, p, dict(CIFAR_CFG), {}
    base, var = name.rsplit("_", 1)
    inp, params, c = CS.make_model_case(base)
    cfg, v = dict(c["cfg"]), MODEL_VARIANTS[var]
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    if "num_virtual_nodes" in v:
        params = VR.init_params("zinc", cfg, v["num_virtual_nodes"], g)
    elif var == "dist":
        hp = DR.head_params(cfg["edge_width"], cfg["model_width"], DIST_T, True, seed=3)
        params = dict(params)
        for n, t in zip(DR.HEAD_NAMES[2:], hp[2:]):
            params[n.replace("/", ".")] = t
    elif var == "bias":
        params = ES.init_params("zinc", cfg, g)
    if v.get("edge_channel_type"):
        cfg["edge_channel_type"] = v["edge_channel_type"]
    return "zinc", inp, params, cfg, v


def ref_model(R, name):
    """DCSVDTransformer(...).get_model() of lib/models/zinc/dc.py or lib/models/cifar10/dc.py, the scheme's loss
    (MeanAbsoluteError / SparseCategoricalCrossentropy(from_logits)) plus what the layers passed to add_loss"""
    kind, inp, params, cfg, v = model_inputs(name)
    B, N = inp["graph_matrix"].shape[:2]
    mod = R.zinc if kind == "zinc" else R.cifar10
    kw = dict(model_width=cfg["model_width"], edge_width=cfg["edge_width"], model_height=cfg["model_height"],
              upto_hop=cfg["upto_hop"], max_length=N, num_heads=H, use_svd=False, readout_edges=False,
              edge_channel_type=cfg.get("edge_channel_type", "residual"), num_virtual_nodes=v.get("num_virtual_nodes", 0),
              distance_loss=v.get("distance_loss", 0.), distance_target=v.get("distance_target", 8))
    if kind == "cifar10":
        kw["num_target_labels"] = cfg["num_targets"]
    feed = dict(node_features=inp["node_features"], feature_matrix=inp["feature_matrix"], graph_matrix=inp["graph_matrix"])
    state = {}

    def run(weights):
        m = mod.DCSVDTransformer(**kw)
        with RX.session(feed=feed, weights=weights):
            state["y"] = m.get_model().outputs
        return m.tracked_layers

    tracked = run(_weights_for(run, params))
    y = state["y"]
    losses = R.tf.keras.losses
    if kind == "zinc":
        base_loss = losses.MeanAbsoluteError(name="MAE")(inp["target"], y)
    else:
        base_loss = losses.SparseCategoricalCrossentropy(from_logits=True, name="xentropy")(inp["target"], y)
    extra = RX.added_losses(tracked)
    loss = base_loss if extra is None else base_loss + extra
    out = dict(y=y, loss=loss.reshape(1))
    L = tracked.get_layers_dict()
    bits = {}
    first = L["virtual_node_embedding"] if "virtual_node_embedding" in L else L["node_emb" if kind == "zinc" else "node_mask"]
    bits["node_mask"] = first.output._keras_mask.as_subclass(torch.Tensor)
    if cfg.get("edge_channel_type") == "constrained":
        M = L["virtual_node_expand_mask" if "virtual_node_expand_mask" in L else "adj_expand_mask"].output
        bits["edge_mask"] = M.as_subclass(torch.Tensor).to(torch.uint8)
    if "adj_add_hops" in L:
        bits["distance_target"] = L["adj_add_hops"].output.as_subclass(torch.Tensor).to(torch.int64)
        out["distance_loss"] = L["distance_loss_layer"].metrics["distance_loss"]
    out.update({f"d/{k}": g for k, g in _grads_by_oracle_key(tracked, loss, params).items()})
    return dict(inputs=inp, weights=params, out=out, bits=bits)


def oracle_model(name):
    kind, inp, params, cfg, v = model_inputs(name)
    p = {k: t.to(F64).requires_grad_() for k, t in params.items()}
    nf, fm, adj = inp["node_features"], inp["feature_matrix"], inp["graph_matrix"]
    nv, ect = v.get("num_virtual_nodes", 0), cfg.get("edge_channel_type", "residual")
    out, bits = {}, {}
    if kind == "cifar10":
        y = MO.cifar10_forward(nf, fm, adj, p, cfg)
        loss = MO.sparse_xent_loss(y, inp["target"])
        bits["node_mask"] = O.node_mask_from_masking(nf, -1.0)
    else:
        bits["node_mask"] = O.node_mask_from_features(nf, nv)
        if nv:
            y = VR.forward("zinc", inp, p, cfg, nv)
        elif ect == "bias":
            y, _ = ES.forward("zinc", inp, p, cfg)
        else:
            M = O.constrained_edge_mask(adj.to(F64), H) if ect == "constrained" else None
            y, _, e_f, _ = MO.zinc_forward(nf, fm, adj, p, cfg, return_hidden=True, attn_mask=M)
        loss = MO.mae_loss(y, inp["target"].to(F64))
        if ect == "constrained":
            bits["edge_mask"] = O.constrained_edge_mask(adj, H, nv).to(torch.uint8)
        if "distance_loss" in v:
            tgt = DR.ref_target(adj, DIST_T)
            per_graph = DR.ref_mlp_loss(e_f, tgt, *[p[n.replace("/", ".")] for n in DR.HEAD_NAMES[2:]], cfg.get("activation", "elu"))
            loss = loss + DIST_W * per_graph.mean()
            bits["distance_target"] = tgt
            out["distance_loss"] = per_graph.detach()
    gr = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    out.update(y=y.detach(), loss=loss.detach().reshape(1))
    out.update({f"d/{k}": (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(p, gr)})
    return out, bits


# --------------------------------------------------------------------------------------------- the table -----
FAMILIES = {
    "attn": (ATTN_NAMES, ref_attn, oracle_attn),
    "block": (BLOCK_NAMES, ref_block, oracle_block),
    "ffn": (list(CS.FFN_CASES), ref_ffn, oracle_ffn),
    "stack": (list(STACK_CASES), ref_stack, oracle_stack),
    "model": (MODEL_NAMES, ref_model, oracle_model),
}
ALL_CASES = [(f, n) for f, (names, _, _) in FAMILIES.items() for n in names]


def ref_case(R, family, name):
    return FAMILIES[family][1](R, name)


def packed_ref_case(R, family, name):
    return pack(ref_case(R, family, name), CAP[family])


def oracle_case(family, name):
    return FAMILIES[family][2](name)
