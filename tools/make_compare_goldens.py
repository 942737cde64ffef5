"""Chooses the seeds of the comparison library's test inputs and records them in tests/golden/compare_cases.npz.

For every case of tests/compare_cases.py (the search shapes, the ragged batch's pairs, the banded pairs) the float64 restatement
(tests/compare_ref.py) alone judges a seed: for D >= 2 the smallest margin of a decision on the path -- best predecessor against second
best -- must be at least 1e-9 of dist_total; D = 1 inputs are exact in double and take seed 0 with no filter.  The first seed that
passes is recorded with its margin, dist_total and path length; the tests rebuild the inputs from the seed.

    python tools/make_compare_goldens.py            # writes the fixture
    python tools/make_compare_goldens.py --check    # compares with the committed one"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import compare_cases as cc  # noqa: E402


def build():
    rows = []
    for name, Ta, Tb, D, band in cc.case_list():
        seed, s = cc.first_good_seed(Ta, Tb, D, band)
        rows.append((name, seed, s["path_margin"], s["dist_total"], len(s["path"])))
        rel = s["path_margin"] / s["dist_total"] if s["dist_total"] else float("inf")
        print(f"{name:>18}: seed {seed:3d}  n_path {len(s['path']):5d}  dist_total {s['dist_total']:.6g}  smallest margin on the path {s['path_margin']:.3e} ({rel:.1e} of dist_total)")
    return dict(names=np.array([r[0] for r in rows]), seeds=np.array([r[1] for r in rows], np.int64), path_margins=np.array([r[2] for r in rows], np.float64),
                dist_totals=np.array([r[3] for r in rows], np.float64), n_paths=np.array([r[4] for r in rows], np.int64))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    g = build()
    if args.check:
        have = np.load(cc.GOLDEN, allow_pickle=False)
        for k, v in g.items():
            assert np.array_equal(have[k], v), k
        print("committed fixture matches")
        return
    np.savez_compressed(cc.GOLDEN, **g)
    print(f"wrote {cc.GOLDEN} ({os.path.getsize(cc.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
