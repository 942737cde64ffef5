"""The case matrix of tests/test_gpu_denoiser_kernels.py and tests/test_denoiser_kernel_ref_host.py: geometries, lengths and the seeded data
of every pass of csrc/denoiser.hip, the smallest at which each path of a kernel exists (B <= 3, at most a few dozen frames)."""
from __future__ import annotations

import numpy as np

from kernel_ref import rng_of

f32 = np.float32

# (filter_length, hop): n_overlap 2, 4, 8 with bins 33, 65, 129 and Cpad 96, 160, 288; (1024, 256): bins 513, three trips of the 256-thread bin loop
SMALL_GEOMS = [(64, 32), (128, 32), (256, 32)]
GEOMS = SMALL_GEOMS + [(1024, 256)]
STRENGTHS = [0.0, 0.1, 0.75, 10.0]        # 0.1: the reference's default, where a fused mag - bias * strength shows; 0: the product is exact
EDGES = [(False, False), (False, True), (True, False), (True, True)]   # (left_real, right_real)


def cpad_of(N):
    return (N + 2 + 31) // 32 * 32


# ---------------------------------------------------------------- reflect-pad
def pad_case(N, hop):
    """n_valid = half (the all-zero rule), half + 1 (the shortest reflectable row), and a length that is no multiple of 4 whose right reflection
    ends inside a float4; R two rows larger than the longest row needs; samples past n_valid[b] are NaN (they must not be read)."""
    half = N // 2
    n_valid = [half, half + 1, half + 2 * hop + 7]
    R = -(-(max(n_valid) + N) // hop) + 2
    wav_len = max(n_valid) + 1
    wav = rng_of(f"dn_pad_{N}_{hop}").standard_normal((3, wav_len)).astype(f32)
    for b, nb in enumerate(n_valid):
        wav[b, nb:] = np.nan
    return dict(n_valid=n_valid, R=R, wav=wav)


def stream_pad_case(N, hop, left_real, right_real, L=None):
    """L: a multiple of hop (launch_stft_pad_stream's rows must match the window; L = half + 1 is therefore refused, and the shortest window
    with a real edge is half + hop)."""
    half = N // 2
    L = L or half + hop
    Rq = (L + (half if left_real else 0) + (half if right_real else 0)) // hop
    seg = rng_of(f"dn_spad_{N}_{hop}_{L}").standard_normal((2, L)).astype(f32)
    return dict(L=L, Rq=Rq, seg=seg)


# ---------------------------------------------------------------- spectral subtraction
def spec_case(N, hop, strength):
    """Gaussian spectra over a few decades, ragged frames (1, R - n_overlap + 1 and one between), and in the first and the last row of the
    longest utterance the special bins: bias far above the magnitude (exact zero), mag == fl(bias * strength) exactly, signed zeros,
    subnormal re / im (squares that underflow to 0 with re != 0; a square that is itself subnormal), one inf and one NaN."""
    nov, bins, Cpad = N // hop, N // 2 + 1, cpad_of(N)
    R = 6 if N == 1024 else 12
    full = R - nov + 1
    frames = [1, full, max(1, full // 2)]
    r = rng_of(f"dn_spec_{N}_{hop}")
    spec = (r.standard_normal((3, R, Cpad)) * 10.0 ** r.uniform(-3, 2, (3, R, 1))).astype(f32)
    bias = np.abs(r.standard_normal(bins)).astype(f32)
    bias[3] = f32(1e6)
    s = f32(strength)
    for f in (0, full - 1):
        re, im = spec[1, f, :bins], spec[1, f, bins:2 * bins]
        re[4], im[4] = bias[4] * s, 0.0                 # mag == fl(bias * strength): md = +0
        re[5], im[5] = -0.0, 0.0
        re[6], im[6] = -0.0, -1.5
        re[7], im[7] = 1e-40, -3e-42                    # both squares underflow to 0: mag = 0, sc = 0, out = (+0, -0)
        re[8], im[8] = 1e-20, 1e-39                     # re * re is subnormal: the root of a subnormal
        re[9], im[9] = np.inf, 1.0
        re[10], im[10] = 2.0, np.nan
        re[11], im[11] = 3e-39, 4e-39                   # subnormal components, squares underflow
    return dict(R=R, Cpad=Cpad, bins=bins, nov=nov, frames=frames, spec=spec, bias=bias)


def bias_case(N):
    """One spectrum row: Gaussians over 40 decades (squares from the subnormals to overflow: the root's scaling paths), then the special bins
    of spec_case."""
    bins = N // 2 + 1
    r = rng_of(f"dn_bias_{N}")
    row = (r.standard_normal(2 * bins) * 10.0 ** r.uniform(-21, 19.5, 2 * bins)).astype(f32)
    re, im = row[:bins], row[bins:]
    re[1:8] = [0.0, -0.0, 1e-40, 1e-20, np.inf, 2.0, 3e-39]
    im[1:8] = [0.0, -1.5, -3e-42, 1e-39, 1.0, np.nan, 4e-39]
    return row


# ---------------------------------------------------------------- overlap-add normalisation
PCM_RAILS = np.array([-32769, -32768, -32767.5, 32767, 32767.5, 1e9, np.nan], np.float64)   # v * 32768
PCM_RAILS_WANT = [-32768, -32768, -32767, 32767, 32767, 32767, -32768]                      # trunc, saturated; NaN: fmaxf's rule


def window_sq(N, hop, holes):
    """The squared periodic Hann window in float64; holes: every hop-block's first hop / 4 terms are 0 and the next is 1e-40, so the envelope is
    0 on a quarter of the positions and positive but under FLT_MIN on one per hop (neither is divided)."""
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)) ** 2
    if holes:
        w = w.reshape(N // hop, hop).copy()
        w[:, :hop // 4] = 0.0
        w[:, hop // 4] = 1e-40
        w = w.reshape(N)
    return w


def ola_case(N, hop, holes=False, odd=False):
    """Rows: full length, ragged (an odd length), pass-through (n_valid <= half, carrying the PCM rails).  n = the longest row (odd: one more,
    so n % 4 == 1).  y positions the kernel may not read, and `in` of the rows that are not passed through, are NaN.  With holes the rails
    also sit in y of row 0 on positions whose envelope is 0 (v = y * n_overlap exactly)."""
    half, nov = N // 2, N // hop
    n0 = 6 * hop if N <= 256 else 4 * hop
    n = n0 + (1 if odd else 0)
    n_valid = [n0, n0 - hop - 5, min(half, 24)]
    frames = [nb // hop + 1 for nb in n_valid]
    R = max(frames) + nov - 1
    r = rng_of(f"dn_ola_{N}_{hop}_{holes}")
    y = np.full((3, R * hop), np.nan, f32)
    inp = np.full((3, n), np.nan, f32)
    for b, nb in enumerate(n_valid[:2]):
        y[b, half:half + nb] = r.standard_normal(nb).astype(f32) * f32(0.2)
    rails = (PCM_RAILS / 32768).astype(f32)
    inp[2, :n_valid[2]] = r.standard_normal(n_valid[2]).astype(f32)
    inp[2, 2:2 + len(rails)] = rails
    if holes:
        i0 = 2 * hop                                   # sample i sits at padded position p = i + half, half % hop == 0: p % hop < hop / 4
        assert len(rails) <= hop // 4
        y[0, i0 + half:i0 + half + len(rails)] = rails / f32(nov)
    return dict(n=n, n_valid=n_valid, frames=frames, R=R, y=y, inp=inp, win_sq=window_sq(N, hop, holes))
