"""Write tests/golden/node_embed/*.npz: what the reference's own ZINC model code computes WITH a positional encoding -- the
path tests/reference_cases.py::ref_model leaves out (use_svd=False) -- run unmodified on the eager stand-in (oracle/ref_exec.py)
in fp64, in inference mode (no sign flip):

    zinc_svd  lib.models.zinc.dc.DCSVDTransformer(use_svd=True, 8 of 16 pairs, transform_svd=True, random_neg=True)
    zinc_eig  lib.models.zinc.dc.DCEigTransformer(use_eig=True, 8 of 20 eigenvectors, transform_eig=False, random_neg=True)
    (SVDFeatModel / EigFeatModel, lib/models/graph_model_base.py:284-414)

Each file holds the inputs, the weights under the oracle's keys, the model output, the MAE loss and the parameter gradients.
Deterministic: a second run writes the same values.  Needs the reference tree (EGT_REFERENCE_DIR); nothing of it is written
here, only numbers it computed.

    python tests/golden/make_node_embed_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))           # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import node_embed_reference as NR  # noqa: E402
import reference_cases as RC  # noqa: E402
from oracle import ref_exec as RX  # noqa: E402


def ref_model(R, name):
    inp, params, cfg = NR.model_inputs(name)
    B, N = inp["graph_matrix"].shape[:2]
    kind = NR.CASES[name]["kind"]
    cls = R.zinc.DCSVDTransformer if kind == "svd" else R.zinc.DCEigTransformer
    kw = dict(model_width=cfg["model_width"], edge_width=cfg["edge_width"], model_height=cfg["model_height"], upto_hop=cfg["upto_hop"],
              max_length=N, num_heads=RC.H, readout_edges=False, num_virtual_nodes=0, random_neg=True)
    if kind == "svd":
        kw.update(use_svd=True, num_svd_features=cfg["num_svd_features"], sel_svd_features=cfg["sel_svd_features"], transform_svd=True)
    else:
        kw.update(use_eig=True, num_eig_features=cfg["num_eig_features"], sel_eig_features=cfg["sel_eig_features"], transform_eig=False)
    feed = {k: inp[k] for k in ("node_features", "feature_matrix", "graph_matrix", NR.PE_KEY[kind])}
    state = {}

    def run(weights):
        m = cls(**kw)
        with RX.session(feed=feed, weights=weights):
            state["y"] = m.get_model().outputs
        return m.tracked_layers

    tracked = run(RC._weights_for(run, params))
    y = state["y"]
    loss = R.tf.keras.losses.MeanAbsoluteError(name="MAE")(inp["target"], y)
    out = dict(y=y, loss=loss.reshape(1))
    out.update({f"d/{k}": g for k, g in RC._grads_by_oracle_key(tracked, loss, params).items()})
    return dict(inputs=inp, weights=params, out=out)


def main():
    os.makedirs(NR.DIR, exist_ok=True)
    with RX.reference() as R:
        for name in NR.CASES:
            case = ref_model(R, name)
            flat = {}
            for grp in ("inputs", "weights", "out"):
                for k, t in case[grp].items():
                    flat[f"{grp}/{k}"] = torch.as_tensor(t).detach().as_subclass(torch.Tensor).cpu().numpy()
            path = os.path.join(NR.DIR, f"{name}.npz")
            np.savez_compressed(path, **flat)
            print(f"{name}.npz  {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
