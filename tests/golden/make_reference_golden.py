"""Write tests/golden/reference/*.npz: what the reference's own model code computes, run unmodified on the eager stand-in
(oracle/ref_exec.py) in fp64, for every case of tests/reference_cases.py.  Deterministic: a second run writes the same
values.  Needs the reference tree (EGT_REFERENCE_DIR); nothing of it is written here, only numbers it computed.

    python tests/golden/make_reference_golden.py [family[:name] ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))           # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import reference_cases as RC  # noqa: E402
from oracle import ref_exec as RX  # noqa: E402


def main(argv):
    want = [a.split(":") for a in argv]
    os.makedirs(RC.REF_DIR, exist_ok=True)
    total = 0
    with RX.reference() as R:
        for family, name in RC.ALL_CASES:
            if want and not any(w[0] == family and (len(w) == 1 or w[1] == name) for w in want):
                continue
            path = os.path.join(RC.REF_DIR, f"{family}_{name}.npz")
            np.savez_compressed(path, **RC.packed_ref_case(R, family, name))
            total += os.path.getsize(path)
            print(f"{family}_{name}.npz  {os.path.getsize(path)} bytes")
    print(f"{total} bytes written")


if __name__ == "__main__":
    main(sys.argv[1:])
