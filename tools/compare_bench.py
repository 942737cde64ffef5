#!/usr/bin/env python3
"""The comparison library (libe2etts_compare.so) at the bench shape: B = 32 pairs of about 768 x 800 frames of 80-bin log-mel, 13
cepstra, the mels resident in HBM.  The three kernels -- cepstra (both sides), search, walk -- are timed with HIP events
(e2ecmp_profile_read), repeated after --warmup calls until --fill-seconds of wall clock are filled; medians and [min, max].  Beside
them, as context only: the float64 restatement of tests/compare_ref.py on the CPU for one pair (numpy, one anti-diagonal at a time) and
a plain-Python DP loop over the same cost matrix.  Prints one JSON line.  Nothing in the tests depends on these times."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def mels(B, T, lens, n_mel, seed):
    """Smooth random log-mel tracks: a low-pass random walk per bin around -5."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((B, T, n_mel)).astype(np.float32)
    for t in range(1, T):
        x[:, t] = 0.9 * x[:, t - 1] + 0.44 * x[:, t]
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return (2.0 * x - 5.0).astype(np.float32)


def python_dp(d):
    Ta, Tb = d.shape
    D = [[0.0] * Tb for _ in range(Ta)]
    rows = d.tolist()
    for i in range(Ta):
        for j in range(Tb):
            if i == 0 and j == 0:
                D[i][j] = rows[0][0]
                continue
            best = D[i - 1][j - 1] if i and j else float("inf")
            if i and D[i - 1][j] < best:
                best = D[i - 1][j]
            if j and D[i][j - 1] < best:
                best = D[i][j - 1]
            D[i][j] = rows[i][j] + best
    return D[-1][-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames-a", type=int, default=768)
    ap.add_argument("--frames-b", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fill-seconds", type=float, default=3.0)
    ap.add_argument("--band", type=int, default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    from e2e_tts_amd import compare as cmplib
    B, n_mel = a.batch, 80
    rng = np.random.Generator(np.random.PCG64(1))
    la = rng.integers(a.frames_a - 40, a.frames_a + 1, B)
    lb = rng.integers(a.frames_b - 40, a.frames_b + 1, B)
    la[0], lb[0] = a.frames_a, a.frames_b
    ma, mb = mels(B, a.frames_a, la, n_mel, 2), mels(B, a.frames_b, lb, n_mel, 3)
    f0a = np.where(rng.random((B, a.frames_a)) > 0.3, rng.uniform(90, 300, (B, a.frames_a)), 0).astype(np.float32)
    f0b = np.where(rng.random((B, a.frames_b)) > 0.3, rng.uniform(90, 300, (B, a.frames_b)), 0).astype(np.float32)
    da, db, fa, fb = (torch.from_numpy(v).cuda() for v in (ma, mb, f0a, f0b))
    torch.cuda.synchronize()
    c = cmplib.Comparator(n_mel, 13)
    c.profile_enable(True)
    ms = {"cepstra_two_sides": [], "search": [], "walk": [], "run_wall": []}
    t_begin, i = time.perf_counter(), 0
    while i < a.warmup + 3 or (time.perf_counter() - t_begin < a.fill_seconds and i < 2000):
        c.set_a(da, la, fa)
        cep = c.profile_read()["cepstra"]
        c.set_b(db, lb, fb)
        cep += c.profile_read()["cepstra"]
        t0 = time.perf_counter()
        res = c.run("dtw", a.band)
        wall = (time.perf_counter() - t0) * 1e3
        p = c.profile_read()
        if i >= a.warmup:
            ms["cepstra_two_sides"].append(cep)
            ms["search"].append(p["search"])
            ms["walk"].append(p["walk"])
            ms["run_wall"].append(wall)
        i += 1
    out = {"tool": "compare_bench", "B": B, "frames_a": a.frames_a, "frames_b": a.frames_b, "n_mel": n_mel, "n_cep": 13, "band": a.band, "calls": len(ms["search"]),
           "device_bytes": c.device_bytes(), "mean_n_path": float(np.mean([r["n_path"] for r in res])), "mean_mcd_db": float(np.mean([r["mcd_db"] for r in res]))}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    if not a.no_cpu:
        import compare_ref as cr
        ca, cb = c.features("a")[0, :la[0]], c.features("b")[0, :lb[0]]
        t0 = time.perf_counter()
        want, _ = cr.compare(ca, cb, band=-1 if a.band is None else a.band)
        out["cpu_restatement_one_pair_s"] = round(time.perf_counter() - t0, 4)
        d = cr.cost_matrix(ca, cb)
        t0 = time.perf_counter()
        total = python_dp(d)
        out["cpu_python_dp_loop_one_pair_s"] = round(time.perf_counter() - t0, 4)
        out["pair0_dist_total_equal"] = bool(res[0]["dist_total"] == want["dist_total"] and (a.band is not None or total == want["dist_total"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
