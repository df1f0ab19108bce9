"""Cases of the reference pin of the positional-encoding path (tests/golden/node_embed/*.npz, written by
tests/golden/make_node_embed_golden.py from the reference's own ZINC model classes with use_svd / use_eig): inputs, fp32
parameters under the oracle's keys and the model config, built deterministically; `load` reads a fixture, `oracle` runs
oracle/egt_model_oracle.py on it in fp64.  No test functions here."""
from __future__ import annotations

import os

import numpy as np
import torch

import cases as CS
from oracle import egt_model_oracle as MO

DIR = os.path.join(CS.GOLDEN_DIR, "node_embed")
PE_KEY = {"svd": "singular_vectors", "eig": "eigen_vectors"}
CASES = {
    "zinc_svd": dict(kind="svd", base="zinc_small", pe=dict(use_svd=True, num_svd_features=16, sel_svd_features=8, transform_svd=True)),
    "zinc_eig": dict(kind="eig", base="zinc_small", pe=dict(use_eig=True, num_eig_features=20, sel_eig_features=8, transform_eig=False)),
}


def model_inputs(name):
    """-> (inputs with the encoding tensor, fp32 parameters under the oracle's keys, model config)"""
    c = CASES[name]
    base = CS.MODEL_CASES[c["base"]]
    cfg = dict(base["cfg"], **c["pe"])
    g = torch.Generator().manual_seed(4242 + sum(map(ord, name)))
    inp, _, _ = CS.make_model_case(c["base"])
    inp = dict(inp)
    B, N = inp["graph_matrix"].shape[:2]
    real = inp["node_features"] != -1
    T = cfg["num_svd_features"] if c["kind"] == "svd" else cfg["num_eig_features"]
    pe = torch.randn(B, N, T, 2, generator=g) if c["kind"] == "svd" else torch.randn(B, N, T, generator=g)
    pe[~real] = 0.0
    inp[PE_KEY[c["kind"]]] = pe
    return inp, MO.init_zinc_params(cfg, dtype=torch.float32, generator=g), cfg


def load(name):
    z = np.load(os.path.join(DIR, f"{name}.npz"))
    out = {"inputs": {}, "weights": {}, "out": {}}
    for k in z.files:
        grp, key = k.split("/", 1)
        out[grp][key] = torch.from_numpy(z[k])
    return out


def oracle(fix, name):
    """{y, loss, d/<key>} of the fp64 oracle on a fixture's inputs and weights"""
    c = CASES[name]
    cfg = dict(CS.MODEL_CASES[c["base"]]["cfg"], **c["pe"])
    inp = fix["inputs"]
    p = {k: v.double().requires_grad_() for k, v in fix["weights"].items()}
    y = MO.zinc_forward(inp["node_features"], inp["feature_matrix"], inp["graph_matrix"], p, cfg,
                        pe={PE_KEY[c["kind"]]: inp[PE_KEY[c["kind"]]].double()})
    loss = MO.mae_loss(y, inp["target"].double())
    gs = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    out = dict(y=y.detach(), loss=loss.detach().reshape(1))
    out.update({f"d/{k}": (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), gs)})
    return out, cfg
