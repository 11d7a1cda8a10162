#!/usr/bin/env python3
"""tests/golden/dl_kernels.npz: the eight length-scale derivatives build_dK / build_dKreg use (families A, B, C) evaluated
by the REFERENCE's own compiled Fortran (oracle/_ref, build container only) at 100 random arguments per family.
Data only: inputs and expected outputs.
Usage:  python tests/golden/make_dl_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.oracle import DL_NAMES, Ref  # noqa: E402


def main():
    ref = Ref()
    rng = np.random.default_rng(3)
    out = {"names": np.array(list(DL_NAMES.values()))}
    for fam in "ABC":
        args, vals = [], []
        for _ in range(100):
            a = rng.uniform(-3, 3, 4)
            lx, ly = rng.uniform(0.3, 2, 2)
            args.append([*a, lx, ly])
            vals.append([ref.scalar(fam, name, *a, lx, ly) for name in DL_NAMES.values()])
        out[fam + "_args"] = np.array(args)          # (x_a, y_a, x_b, y_b, lx, ly)
        out[fam + "_values"] = np.array(vals)        # columns in the order of `names`
    np.savez(os.path.join(HERE, "dl_kernels.npz"), **out)
    print("wrote dl_kernels.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
