"""Write tests/golden/xtalk/*.npz: the reference's ZINC model with node2edge_xtalk / edge2node_xtalk, run unmodified on the eager
stand-in (oracle/ref_exec.py) in fp64, for every case of tests/xtalk_cases.py MODEL_CASES.  Deterministic: a second run writes
the same values.  Needs the reference tree (EGT_REFERENCE_DIR); nothing of it is written here, only numbers it computed.

    python tests/golden/make_xtalk_golden.py [name ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))           # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import xtalk_cases as XC  # noqa: E402
from oracle import ref_exec as RX  # noqa: E402


def main(argv):
    os.makedirs(XC.XT_DIR, exist_ok=True)
    total = 0
    with RX.reference() as R:
        for name in XC.MODEL_CASES:
            if argv and name not in argv:
                continue
            path = XC.fixture_path(name)
            np.savez_compressed(path, **XC.packed_ref_model(R, name))
            total += os.path.getsize(path)
            print(f"{name}.npz  {os.path.getsize(path)} bytes")
    print(f"{total} bytes written")


if __name__ == "__main__":
    main(sys.argv[1:])
