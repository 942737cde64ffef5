#!/usr/bin/env python3
"""What the ORDER OF SUMMATION of the denoiser's two exact-fp32 GEMMs costs, on the CPU: tests/denoiser_ref.py's row form with every
output accumulated as conv_gemm accumulates it -- ONE float32 chain per output, in the kernel's order of terms (32-channel chunk, then
tap, then channel) -- instead of BLAS's blocked sums, compared with the reference's float64 run stored in tests/golden/denoiser.npz.

Variants: the forward / inverse GEMM exact (float64, rounded once) to see which one carries the error; the forward / inverse GEMM as
one chain per tap, the taps added afterwards (what engine_denoise.hip: denoise_impl does for the inverse).

On fixture (c) (the tiny vocoder's audio, which has a constant offset) this printed, mean-L1 / max against float64:
    one chain each            5.888e-08 / 7.739e-07     (MI355X, inverse as one KW = 4 convolution: 5.934e-08 / 7.888e-07)
    forward exact             5.667e-08 / 7.118e-07
    inverse exact             1.480e-08 / 8.048e-08     -> the inverse's chain of 4 224 terms is what costs
    forward per tap           5.737e-08 / 6.994e-07
    inverse per tap           2.600e-08 / 2.001e-07     (MI355X, inverse as four accumulated launches: 2.595e-08 / 2.448e-07)
    both per tap              2.249e-08 / 2.382e-07
and for (a) / (b) with the inverse per tap 4.407e-08 / 4.243e-08 (MI355X: 4.425e-08 / 4.195e-08).

Usage:  python tools/experiments/denoiser_sum_order.py        (a minute or two: the chains are Python loops over K)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoiser_ref as dr  # noqa: E402
from e2e_tts_amd import denoiser as dn  # noqa: E402


def chain(A, W, order):
    """A [M, K] @ W [K, N] with every output one float32 accumulator that takes the terms in `order` (products exact, as an FMA's)."""
    acc = np.zeros((A.shape[0], W.shape[1]), np.float32)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    for k in order:
        acc = (acc.astype(np.float64) + np.outer(A64[:, k], W64[k])).astype(np.float32)
    return acc


def conv_order(Cin, KW):
    """conv_gemm's order of the K = KW * Cin terms of a tap-major weight row: chunk of 32 channels, tap, channel."""
    return [j * Cin + c + i for c in range(0, Cin, 32) for j in range(KW) for i in range(32) if c + i < Cin]


def gemm(A, W, Cin, KW, how):
    if how == "exact":
        return (A.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)
    if how == "per_tap":
        out = None
        for j in range(KW):
            part = chain(A[:, j * Cin:(j + 1) * Cin], W[j * Cin:(j + 1) * Cin], range(Cin))
            out = part if out is None else out + part
        return out
    return chain(A, W, conv_order(Cin, KW))


def denoise(x, bias, strength, fwd, inv, win_sq, hop, forward="chain", inverse="chain"):
    N = fwd.shape[1]
    V, bins, n = N // hop, N // 2 + 1, len(x)
    F = n // hop + 1
    R = F + V - 1
    rows = np.pad(x.astype(np.float32), N // 2, mode="reflect").reshape(R, hop)
    A = np.concatenate([rows[j:j + F] for j in range(V)], axis=1)          # frame f = rows f .. f + V - 1
    spec = dr._subtract(gemm(A, fwd.T.copy(), hop, V, forward), np.asarray(bias), strength, bins)
    C = N + 2
    z = np.zeros((V - 1, C), np.float32)
    pd = np.concatenate([z, spec, z])
    A2 = np.concatenate([pd[j:j + R] for j in range(V)], axis=1)           # row q takes frame q - (V - 1) + j at tap V - 1 - j
    W2 = np.concatenate([inv[:, (V - 1 - j) * hop:(V - j) * hop] for j in range(V)], axis=0)
    return dr._finish(gemm(A2, W2, C, V, inverse).reshape(-1), win_sq, F, N, hop, n)


def report(g, tag, N, V, audio, n_valid, bias, strength, ref64, **kw):
    fwd, inv, win_sq = dn.stft_bases(N, N // V, N)
    d = np.concatenate([np.abs(denoise(audio[b, :nb], bias, strength, fwd, inv, win_sq, N // V, **kw).astype(np.float64) - ref64[b, :nb])
                        for b, nb in enumerate(n_valid)])
    print(f"({tag}) {kw or 'one chain each'}: mean-L1 {d.mean():.3e} max {d.max():.3e}", flush=True)


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "denoiser.npz"))
    ca = g["c_audio"]
    for kw in ({}, dict(forward="exact"), dict(inverse="exact"), dict(forward="per_tap"), dict(inverse="per_tap"), dict(forward="per_tap", inverse="per_tap")):
        report(g, "c", 1024, 4, ca, [ca.shape[1]] * 2, g["c_bias_spec"], float(g["c_strength"]), g["c_out64"], **kw)
    report(g, "a", 1024, 4, g["a_audio"], list(g["a_n_valid"]), g["a_bias"], 0.1, g["a_out64_s0"], inverse="per_tap")
    report(g, "b", 512, 2, g["b_audio"], list(g["b_n_valid"]), g["b_bias"], 0.1, g["b_out64_s0"], inverse="per_tap")


if __name__ == "__main__":
    main()
