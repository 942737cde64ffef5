#!/usr/bin/env python3
"""Times the vocoder critic (libe2etts_critic.so) on one GPU: the fused call ``Critic.run`` at B = 32 x 196 608 samples and at B = 1, wall
time per call and the per-layer-class times the library takes from HIP events around its launches (dense conv_gemm layers, grouped
layers, everything else), the grouped kernel's TFLOP/s against the 157.3 TFLOP/s fp32 MFMA peak of an MI355X, and the one comparison
worth recording: the grouped layers (MSD layers 2 - 6) on the grouped kernel against the same layers run as block-diagonal dense
``conv_gemm`` launches (the same tables with groups = 1; a dense layer's time does not depend on which weights are zero).

Synthetic weights and noise input: timings do not depend on the values.  Prints one JSON line per measurement.

Usage:  python tools/critic_bench.py [--B 32] [--n 196608] [--steps 3] [--skip-dense]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from e2e_tts_amd import critic as crit, synth_weights as sw  # noqa: E402

PEAK_TFLOPS = 157.3


def out_len(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def grouped_flops(cfg, n):
    """2 x MACs of the grouped layers of every scale discriminator for one row of n samples."""
    total = 0
    for scale in range(int(cfg["n_scales"])):
        t = n
        for _ in range(scale):
            t = out_len(t, 4, 2, 2)
        cin = 1
        for cout, k, s, g, pad in cfg["msd"]:
            t = out_len(t, k, s, pad)
            if g > 1:
                total += 2 * t * cout * (cin // g) * k
            cin = cout
    return total


def measure(name, cfg, B, n, steps, seed=3):
    import torch
    c = crit.Critic(cfg)
    c.load(*sw.synth_critic_state(seed, cfg))
    c.profile_enable(True)
    g = torch.Generator(device="cuda").manual_seed(1)
    y = 0.1 * torch.randn((B, n), device="cuda", generator=g)
    x = y + 0.01 * torch.randn((B, n), device="cuda", generator=g)
    lens = np.full(B, n, np.int64)
    torch.cuda.synchronize()
    c.run(y, lens, x, lens)   # warm-up: workspaces grow here
    wall, cls = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        c.run(y, lens, x, lens)
        wall.append((time.perf_counter() - t0) * 1e3)
        cls.append(c.profile_read())
    ms = {k: float(np.median([d[k] for d in cls])) for k in cls[0]}
    rec = dict(name=name, B=B, n=n, steps=steps, wall_ms=float(np.median(wall)), device_bytes=c.device_bytes(), **{k + "_ms": v for k, v in ms.items()})
    fl = grouped_flops(cfg, n) * 2 * B   # both sides
    if fl and ms["grouped"] > 0:
        rec["grouped_tflops"] = fl / ms["grouped"] / 1e9
        rec["grouped_share_of_peak"] = rec["grouped_tflops"] / PEAK_TFLOPS
    c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--n", type=int, default=196608)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-dense", action="store_true", help="leave out the block-diagonal conv_gemm comparison")
    a = ap.parse_args()
    full = crit.default_config()
    measure("fused", full, a.B, a.n, a.steps)
    measure("fused_b1", full, 1, a.n, a.steps)
    if a.skip_dense:
        return
    # the scale discriminators alone, as they are and with every grouped layer as one dense (block-diagonal) layer
    msd = dict(full, periods=[])
    grouped = measure("msd_grouped_kernel", msd, a.B, a.n, a.steps)
    dense_cfg = dict(msd, msd=[(co, k, s, 1, p) for co, k, s, g, p in full["msd"]])
    dense = measure("msd_block_diagonal_conv_gemm", dense_cfg, a.B, a.n, a.steps)
    # what the five layers cost as dense launches: the dense class of that run less the one layer that is dense in both
    as_dense = dense["dense_ms"] - grouped["dense_ms"]
    print(json.dumps(dict(name="grouped_layers", B=a.B, n=a.n, grouped_kernel_ms=grouped["grouped_ms"], block_diagonal_conv_gemm_ms=as_dense,
                          grouped_kernel_is_faster=bool(grouped["grouped_ms"] < as_dense), ratio=as_dense / grouped["grouped_ms"])), flush=True)


if __name__ == "__main__":
    main()
