"""Times e2e_tts_amd.stats.CorpusStats.add (libe2etts_stats.so) at B = 32 and B = 256 rows of T = 768 frame energies, beside the reference's
arithmetic on the host: np.percentile + the IQR rule + sklearn's StandardScaler.partial_fit per row, then the min / max pass -- in one
process, and over 16 worker processes that each take a share of the rows and merge at the end.  Also prints the measured ratios of the
GPU's figures to the bars of tests/stats_ref.py on the fixture's corpora.  The figures of profiles/stats/README.md come from here.

    python tools/stats_bench.py [--iters 50]"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rows(B: int, T: int) -> np.ndarray:
    import stats_cases as sc
    rng = sc.rng_of(f"bench{B}x{T}")
    return np.stack([sc.energy_row(rng, T) for _ in range(B)])


def host_share(x: np.ndarray):
    """The reference's first pass on a share of the rows -> (n, mean, var, raw min, raw max)."""
    from sklearn.preprocessing import StandardScaler
    sc = StandardScaler()
    for v in x:
        p25, p75 = np.percentile(v, 25), np.percentile(v, 75)
        lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
        kept = v[np.logical_and(v > lower, v < upper)]
        if len(kept):
            sc.partial_fit(kept.reshape(-1, 1))
    return int(sc.n_samples_seen_), float(sc.mean_[0]), float(sc.var_[0]), float(x.min()), float(x.max())


def host_time(x: np.ndarray, workers: int, iters: int) -> float:
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    if workers == 1:
        host_share(x)   # warm: imports
        t0 = time.perf_counter()
        for _ in range(iters):
            host_share(x)
        return (time.perf_counter() - t0) / iters * 1e3
    shares = np.array_split(x, workers)
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("spawn")) as ex:
        list(ex.map(host_share, shares))   # warm: imports
        t0 = time.perf_counter()
        for _ in range(iters):
            list(ex.map(host_share, shares))
        return (time.perf_counter() - t0) / iters * 1e3


def bar_ratios():
    """The worst ratio of |GPU - reference| to its bar over the fixture's corpora, per figure."""
    import stats_cases as sc
    import stats_ref as sr
    from e2e_tts_amd import stats as stlib
    from test_stats_host import want_stats
    gold, st = sc.load(), stlib.CorpusStats()
    worst = {}
    for name, utts in sc.corpora().items():
        st.reset()
        for key in ("energy", "pitch", "f0"):
            x, lens = sc.batch(utts, key)
            st.add(**{key: x}, lens=lens)
        got, want, ref = st.result(), want_stats(gold, name), sr.corpus(utts)
        for key in ("f0", "energy", "pitch"):
            N, sa, tot = ref["_bars"][key]
            m, s = want[key]["mean"], want[key]["std"]
            worst["mean"] = max(worst.get("mean", 0.0), abs(got[key]["mean"] - m) / (sr.mean_bar(N, sa, tot) * abs(m)))
            if s not in (0.0, 1.0):
                worst["std"] = max(worst.get("std", 0.0), abs(got[key]["std"] - s) / (sr.std_bar(N, m, s) * s))
                if key != "f0":
                    for k in ("min", "max"):
                        worst[k] = max(worst.get(k, 0.0), abs(got[key][k] - want[key][k]) / sr.z_bar(want[key][k], N, sa, tot, m, s))
    st.close()
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    T = 768
    data = {B: rows(B, T) for B in (32, 256)}
    host = {B: (host_time(x, 1, max(2, args.iters // 10)), host_time(x, 16, max(2, args.iters // 10))) for B, x in data.items()}   # before the GPU is opened
    import torch
    from e2e_tts_amd import stats as stlib
    st = stlib.CorpusStats()
    st.profile_enable(True)
    for B, x in data.items():
        xd = torch.from_numpy(x).cuda()
        lens = np.full(B, T, np.int64)
        for _ in range(5):
            st.add(energy=xd, lens=lens)
        st.sync()
        rows_ms, merge_ms, wall = [], [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            st.add(energy=xd, lens=lens)
            st.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            p = st.profile_read()
            rows_ms.append(p["rows"])
            merge_ms.append(p["merge"])
        t0 = time.perf_counter()
        for _ in range(args.iters):
            st.add(energy=xd, lens=lens)
        enq = (time.perf_counter() - t0) / args.iters * 1e3
        st.sync()
        print(f"B={B} T={T}: rows kernel {np.median(rows_ms):.4f} ms, merge kernel {np.median(merge_ms):.4f} ms, add + sync wall {np.median(wall):.4f} ms, "
              f"add enqueue alone {enq:.4f} ms; host numpy + sklearn {host[B][0]:.2f} ms in one process, {host[B][1]:.2f} ms over 16 processes", flush=True)
    st.close()
    print("worst |GPU - reference| / bar over the fixture's corpora:", {k: f"{v:.3g}" for k, v in bar_ratios().items()}, flush=True)


if __name__ == "__main__":
    main()
