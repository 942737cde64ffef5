"""Restatement of the reference's vocoder-bias denoiser (V/denoiser.py: STFT :55-153, Denoiser :156-186) in numpy, two ways.

``denoise_frames``  the textbook form, any dtype: reflect-pad, cut frames, one matrix product with the forward basis, subtract the bias from
                    the magnitudes, one matrix product with the inverse basis, overlap-add, divide by the window envelope, scale, trim.
                    In float64 (with the float32 bases widened, as ``module.double()`` widens its buffers) it is the reference's float64 run.
``denoise_rows``    the form the engine computes (csrc/denoiser.hip): the padded signal as rows of `hop` samples, the forward transform a
                    sum of n_overlap products of row blocks with column blocks of the basis (a "same" convolution with pad = 0), the
                    inverse the same the other way round with the taps reversed (pad = n_overlap - 1), whose output rows ARE the
                    overlap-add.  float32 throughout: what exact-fp32 GEMMs give up to the order of summation.
Both take ONE utterance [n] and handle it alone; a batch is its rows trimmed to their lengths.
"""
from __future__ import annotations

import numpy as np


def envelope(win_sq: np.ndarray, n_frames: int, hop: int) -> np.ndarray:
    """librosa's window_sumsquare as the reference calls it (:12-52, dtype float32): a float32 accumulator that takes the float64 squared
    window of every frame in turn."""
    N = len(win_sq)
    x = np.zeros(N + hop * (n_frames - 1), np.float32)
    for f in range(n_frames):
        x[f * hop:f * hop + N] += win_sq          # float64 sum, stored as float32
    return x


def _subtract(spec, bias, strength, bins):
    re, im = spec[:, :bins], spec[:, bins:2 * bins]
    mag = np.sqrt(re ** 2 + im ** 2)
    md = np.maximum(mag - bias.astype(spec.dtype) * spec.dtype.type(strength), 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = np.where(mag > 0, md / mag, 0).astype(spec.dtype)     # mag_d cos / sin(atan2(im, re)) = (re, im) mag_d / mag
    return np.concatenate([re * sc, im * sc], axis=1)


def _finish(ola, win_sq, n_frames, N, hop, n):
    env = envelope(win_sq, n_frames, hop)
    ok = env > np.finfo(np.float32).tiny
    ola = ola.copy()
    ola[ok] = ola[ok] / env[ok]
    ola *= ola.dtype.type(N / hop)
    return ola[N // 2:N // 2 + n]


def denoise_frames(x, bias, strength, fwd, inv, win_sq, hop, dtype=np.float64):
    N = fwd.shape[1]
    bins = N // 2 + 1
    x = np.asarray(x, dtype)
    n = len(x)
    if n % hop or n <= N // 2:
        raise ValueError(f"{n} samples: need a multiple of hop {hop} above filter_length / 2 = {N // 2}")
    p = np.pad(x, N // 2, mode="reflect")
    F = n // hop + 1
    frames = np.stack([p[f * hop:f * hop + N] for f in range(F)])
    spec = _subtract(frames @ fwd.astype(dtype).T, np.asarray(bias), strength, bins)
    parts = spec @ inv.astype(dtype)                                   # [F, N]: frame f lands at samples f * hop ..
    ola = np.zeros(N + hop * (F - 1), dtype)
    for f in range(F):
        ola[f * hop:f * hop + N] += parts[f]
    return _finish(ola, win_sq, F, N, hop, n)


def denoise_rows(x, bias, strength, fwd, inv, win_sq, hop):
    N = fwd.shape[1]
    V, bins = N // hop, N // 2 + 1
    x = np.asarray(x, np.float32)
    n = len(x)
    if n % hop or n <= N // 2:
        raise ValueError(f"{n} samples: need a multiple of hop {hop} above filter_length / 2 = {N // 2}")
    F = n // hop + 1
    R = F + V - 1
    rows = np.pad(x, N // 2, mode="reflect").reshape(R, hop)
    spec = np.zeros((F, N + 2), np.float32)
    for j in range(V):                                                 # frame f = rows f .. f + V - 1
        spec += rows[j:j + F] @ fwd[:, j * hop:(j + 1) * hop].T
    spec = _subtract(spec, np.asarray(bias), strength, bins)
    z = np.zeros((V - 1, N + 2), np.float32)
    padded = np.concatenate([z, spec, z])                              # zero frames before the first and after the last
    out = np.zeros((R, hop), np.float32)
    for j in range(V):                                                 # output row q takes frame q - (V - 1) + j at tap V - 1 - j
        k = V - 1 - j
        out += padded[j:j + R] @ inv[:, k * hop:(k + 1) * hop]
    return _finish(out.reshape(-1), win_sq, F, N, hop, n)


def denoise_batch(fn, audio, n_valid, *args, **kw):
    """Rows denoised alone over their valid samples, zeros past them; rows at or under filter_length / 2 passed through (the engine's rule)."""
    out = np.zeros(audio.shape, np.result_type(kw.get("dtype", np.float32)))
    N = args[2].shape[1]
    for b, nb in enumerate(n_valid):
        nb = int(nb)
        out[b, :nb] = audio[b, :nb] if nb <= N // 2 else fn(audio[b, :nb], *args, **kw)
    return out
