"""The inputs of the comparison library's tests, made from seeds: tools/make_compare_goldens.py chooses the seeds (with the float64
restatement alone) and records them with their margins in tests/golden/compare_cases.npz; the host and the GPU tests rebuild the inputs
from what is recorded there."""
import os

import numpy as np

import compare_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "compare_cases.npz")

PAIRS = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 64), (64, 65), (65, 63), (255, 257), (257, 256), (300, 40), (40, 300), (513, 511)]
DIMS = (1, 13, 32)
RAGGED_A, RAGGED_B, RAGGED_D = (257, 64, 1), (5, 300, 1), 13
BANDS = (1, 2, 8)
BAND_PAIRS = [(63, 64), (300, 40), (40, 300), (257, 256), (7, 1)]
MIN_MARGIN = 1e-9      # of dist_total: the smallest margin of a decision on the path, for D >= 2
MAX_SEED = 200


def case_list():
    """(name, Ta, Tb, D, band) of every seeded case: the search shapes, the ragged batch's pairs, the banded pairs."""
    out = [(f"s{Ta}x{Tb}x{D}", Ta, Tb, D, -1) for Ta, Tb in PAIRS for D in DIMS]
    out += [(f"r{Ta}x{Tb}x{RAGGED_D}", Ta, Tb, RAGGED_D, -1) for Ta, Tb in zip(RAGGED_A, RAGGED_B)]
    out += [(f"b{band}_{Ta}x{Tb}x13", Ta, Tb, 13, band) for Ta, Tb in BAND_PAIRS for band in BANDS]
    return out


def features(Ta, Tb, D, seed):
    """Gaussian features a [Ta, D] and a warped, noisy copy b [Tb, D], float32.  D == 1: both rounded to multiples of 1 / 256, so every
    cost and every sum of costs is exact in double and exact ties abound."""
    rng = np.random.default_rng([seed, Ta, Tb, D])
    a = rng.standard_normal((Ta, D))
    steps = rng.uniform(0.2, 1.8, Tb)
    pos = np.cumsum(steps) - steps[0]
    pos = pos / max(pos[-1], 1e-9) * (Ta - 1) if Tb > 1 else np.zeros(1)
    lo = np.clip(np.floor(pos).astype(int), 0, Ta - 1)
    hi = np.clip(lo + 1, 0, Ta - 1)
    w = (pos - lo)[:, None]
    b = (1 - w) * a[lo] + w * a[hi] + 0.3 * rng.standard_normal((Tb, D))
    if D == 1:
        a, b = np.round(a * 256) / 256, np.round(b * 256) / 256
    return a.astype(np.float32), b.astype(np.float32)


def verdict(Ta, Tb, D, band, seed):
    """(accepted, search dict) of one seed under the restatement alone."""
    a, b = features(Ta, Tb, D, seed)
    s = cr.search(cr.cost_matrix(a, b), band)
    if s["status"]:
        return False, s
    return (D == 1 or s["path_margin"] >= MIN_MARGIN * s["dist_total"]), s


def first_good_seed(Ta, Tb, D, band):
    for seed in range(MAX_SEED):
        ok, s = verdict(Ta, Tb, D, band, seed)
        if ok:
            return seed, s
    raise RuntimeError(f"no seed below {MAX_SEED} passes the margin filter for {(Ta, Tb, D, band)}")


def load():
    """name -> dict(seed, path_margin, dist_total, n_path) of tests/golden/compare_cases.npz."""
    g = np.load(GOLDEN, allow_pickle=False)
    return {str(n): dict(seed=int(s), path_margin=float(m), dist_total=float(d), n_path=int(k))
            for n, s, m, d, k in zip(g["names"], g["seeds"], g["path_margins"], g["dist_totals"], g["n_paths"])}


def harmonic(n, sr, f0, seed=0):
    """A five-harmonic tone of n samples with a slow vibrato and a little noise, float32 in [-1, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f = f0 * (1.0 + 0.02 * np.sin(2 * np.pi * 4.0 * t))
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = 0.3 * sum(a * np.sin((k + 1) * ph) for k, a in enumerate([1.0, 0.5, 0.35, 0.2, 0.1])) / 2.15 + 0.002 * rng.standard_normal(n)
    return x.astype(np.float32)
