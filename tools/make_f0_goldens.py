#!/usr/bin/env python3
"""Writes tests/golden/f0_cases.npz: for every case of tests/f0_cases.py the float64 reference's track, chosen candidate index and
path margin per row, so that the reference (tests/f0_ref.py) itself cannot drift unnoticed.  Also prints, per case, the first seed that
passes the seed filter (what tests/f0_cases.py: SEEDS must hold) and the filter's figures.  No GPU needed."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import f0_cases as fc  # noqa: E402


def main():
    out = {}
    for name in fc.CASES:
        seed = fc.first_good_seed(name)
        if seed != fc.SEEDS[name]:
            print(f"{name}: the first passing seed is {seed}, tests/f0_cases.py holds {fc.SEEDS[name]}: correct SEEDS and run again")
            return 1
        case = fc.build(name)
        refs = fc.reference(case)
        share, margin, rows, close = fc.verdict(refs)
        print(f"{name}: seed {seed}, frames left out {share:.3f}, smallest path margin {margin:.3e}, rows compared end to end {rows}")
        T = max(r["T"] for r in refs)
        f0, idx = np.zeros((len(refs), T), np.float64), np.zeros((len(refs), T), np.int8)
        for b, r in enumerate(refs):
            f0[b, :r["T"]], idx[b, :r["T"]] = r["f0"], r["index"]
        out[name + ".f0"], out[name + ".index"] = f0, idx
        out[name + ".frames"] = np.array([r["T"] for r in refs], np.int64)
        out[name + ".path_margin"] = np.array([r["path_margin"] for r in refs], np.float64)
    path = os.path.join(ROOT, "tests", "golden", "f0_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
