#!/usr/bin/env python3
"""Writes tests/golden/model_egt_simple_small.npz: prediction, loss and every parameter gradient of the EGT-Simple composition
in tests/egt_simple_ref.py (fp64) on its small seeded case.  Run from the repository root: python tests/golden/make_egt_simple_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import egt_simple_ref as R  # noqa: E402

if __name__ == "__main__":
    np.savez_compressed(R.GOLDEN, **R.small_case_outputs())
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
