"""Write tests/golden/attn_dropout/*.npz: what the reference's own model code computes with attn_dropout in training mode, run
unmodified on the eager stand-in (oracle/ref_exec.py) in fp64 with the keep masks of the kernels' counter stream injected, for the
cases of tests/attn_dropout_cases.py -- one residual block per recipe (rate 0.25 alone; rate 0.1 with random_mask_prob 0.1;
[2, 19, 64], De = 16, one padded graph) and a two-layer ZINC model (model_width 64, edge_width 16, N = 19, rate 0.1).  Deterministic:
a second run writes the same values.  Needs the reference tree (EGT_REFERENCE_DIR); nothing of it is written here, only numbers it
computed.

    python tests/golden/make_attn_dropout_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))           # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import attn_dropout_cases as SC  # noqa: E402
from oracle import ref_exec as RX  # noqa: E402


def main():
    os.makedirs(SC.DIR, exist_ok=True)
    with RX.reference() as R:
        for name, flat in SC.files(R).items():
            path = os.path.join(SC.DIR, name)
            np.savez_compressed(path, **flat)
            size = os.path.getsize(path)
            print(f"{name}  {size} bytes")
            assert size <= SC.MAX_BYTES, f"{name}: {size} bytes is over the limit of {SC.MAX_BYTES}"


if __name__ == "__main__":
    main()
