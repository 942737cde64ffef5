"""The cases of tests/test_gpu_mel_tail.py (and of tests/test_mel_tail_host.py): geometries with 16-, 8-, 4- and 2-frame tiles, T around the tile,
n_mel 4 / 20 / 80 / 128, mel matrices with designed bands, spectra with the values at which the tail can go wrong."""
from __future__ import annotations

import functools
import zlib

import numpy as np

import mel_tail_ref as tr

f32, f64 = np.float32, np.float64
CLIP = f32(1e-5)
# (n_fft, hop): bins 129, 1025, 2049, 4097 -> tiles of 16, 8, 4, 2 frames
GEOMS = [(256, 64), (2048, 512), (4096, 512), (8192, 1024)]
TILES = {256: 16, 2048: 8, 4096: 4, 8192: 2}
N_MELS = [4, 20, 80, 128]
W_CLIP = f32(2.0 ** -30)        # the weight of the clip row: acc = 2^-30 * mag, exactly


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def clip_bin(bins):
    return bins // 3


@functools.lru_cache(maxsize=None)
def basis_of(n_fft, n_mel):
    """[n_mel, bins] float32.  Row 0: the clip row (one bin, weight 2^-30).  n_mel = 4: then the dense row, five bins at the low end, five at the
    high end (one wavefront holds all four: bands at opposite ends of the spectrum).  n_mel >= 20: rows 0 .. 8 have band widths 1 .. 9 (every
    remainder of the four-bin unroll, at starts of every residue mod 4), row 9 is empty, row 10 dense, rows 12 and 13 (one wavefront at every
    tile size) sit at opposite ends, row 11 has explicit zeros inside its band, and the rest are overlapping triangles."""
    bins = n_fft // 2 + 1
    r = rng_of(f"melt_basis_{n_fft}_{n_mel}")
    w = np.zeros((n_mel, bins), f32)

    def fill(m, a, b):   # (a row factor of 1, 0.1 or 0.01: with magnitudes of at least sqrt(1e-9) the small ones put quiet frames under the clip)
        w[m, a:b + 1] = (r.uniform(0.25, 1.0, b - a + 1) * r.choice([1.0, 0.1, 0.01])).astype(f32)

    w[0, clip_bin(bins)] = W_CLIP
    if n_mel == 4:
        fill(1, 0, bins - 1)
        fill(2, 0, 4)
        fill(3, bins - 5, bins - 1)
        return w
    for j in range(1, 9):
        a = (7 * j + j * (bins // 11)) % (bins - 16)
        fill(j, a, a + j)                       # widths 2 .. 9
    fill(10, 0, bins - 1)
    fill(11, 20, 40)
    w[11, 23:37] = 0                            # a band with zeros inside: first and last non-zero bin decide
    fill(12, 0, 4)                              # (its neighbour past the band, bin 5, is where the spectra put an infinite magnitude)
    fill(13, bins - 4, bins - 1)
    n_tri = n_mel - 14
    centres = np.linspace(8, bins - 9, n_tri)
    hw = max(3.0, 1.5 * (centres[1] - centres[0]))     # half-width: neighbours overlap at every geometry
    k = np.arange(bins)
    for i, c in enumerate(centres):
        tri = np.maximum(0.0, 1.0 - np.abs(k - c) / hw)
        w[14 + i] = (tri / hw).astype(f32)
    return w


def t_values(n_fft):
    tile = TILES[n_fft]
    return [tile - 1, tile, tile + 1]


def frames_of(T):
    """Ragged rows: all T frames, one frame, T - 1."""
    return [T, 1, max(T - 1, 1)]


@functools.lru_cache(maxsize=None)
def full_spectrum(n_fft, hop, n_mel):
    """spec [3, tile + 1 + n_overlap - 1, Cpad]: what every launch of this (geometry, n_mel) takes its first T + n_overlap - 1 rows from.  Gaussian
    re / im with a per-frame amplitude over seven decades (so that both sides of the clamp occur); the padding channels and the rows no
    frame reads hold NaN.  The first frames carry the special values: a zero frame, re^2 overflowing, subnormal squares, a NaN bin, and the
    clip row's sum exactly on, one ulp below and one ulp above clip (frames 0 .. 2 of row 0: all three exist at T = tile + 1 >= 3), and (tiles of
    at least 4 frames) a frame with one bin alone whose magnitude a fused sum of squares rounds the other way."""
    bins, nov = n_fft // 2 + 1, n_fft // hop
    cpad = tr.cpad_of(bins)
    T = TILES[n_fft] + 1
    r = rng_of(f"melt_spec_{n_fft}_{n_mel}")
    B, R = 3, T + nov - 1
    spec = np.full((B, R, cpad), np.nan, f32)
    amp = 10.0 ** r.uniform(-7, 0, (B, T, 1))
    spec[:, :T, :2 * bins] = (r.standard_normal((B, T, 2 * bins)) * amp).astype(f32)
    kc = clip_bin(bins)
    spec[1, 0, :2 * bins] = 0                                        # a zero spectrum: every magnitude sqrt(1e-9)
    spec[2, 0, 5] = 3e19                                             # re^2 = inf
    spec[2, 0, bins + 7] = -2.5e19                                   # im^2 = inf
    spec[2, 1, 2] = np.nan                                           # a NaN bin: only the rows whose band holds bin 2
    spec[0, 0, 8:16] = 3e-21                                         # squares in the subnormals (9e-42)
    spec[0, 0, bins + 8:bins + 16] = 1e-23                           # squares that underflow to 0
    t = f32(f64(CLIP) * 2.0 ** 30)                                   # 2^-30 t = clip exactly; the neighbours of t give its neighbours
    for f, v in enumerate((np.nextafter(t, f32(0)), t, np.nextafter(t, f32(np.inf)))):
        spec[0, f, kc], spec[0, f, bins + kc] = v, 0
    if T >= 4:                                                       # one bin alone (the energy IS its magnitude), with (re, im) at which
        spec[2, 2, :2 * bins] = 0                                    # a fused re^2 + im^2 rounds the magnitude the other way
        while True:
            re, im = (r.uniform(50, 200, 64)).astype(f32), (r.uniform(50, 200, 64)).astype(f32)
            hit = np.flatnonzero(tr.magnitudes(re, im) != tr.magnitudes(re, im, "fused_squares"))
            if hit.size:
                spec[2, 2, 10], spec[2, 2, bins + 10] = re[hit[0]], im[hit[0]]
                break
    return spec


def spectrum(n_fft, hop, n_mel, T):
    """(spec [3, T + n_overlap - 1, Cpad], frames [3]) of one launch; the rows past T frames are all NaN (never read)."""
    spec = full_spectrum(n_fft, hop, n_mel)[:, :T + n_fft // hop - 1].copy()
    spec[:, T:] = np.nan
    return spec, frames_of(T)


@functools.lru_cache(maxsize=None)
def full_reference(n_fft, hop, n_mel, mut=None):
    T = TILES[n_fft] + 1
    return tr.tail_f32(full_spectrum(n_fft, hop, n_mel), [T] * 3, T, n_fft // 2 + 1, basis_of(n_fft, n_mel), CLIP, mut)


def reference(n_fft, hop, n_mel, T, mut=None):
    """Computed once per (geometry, n_mel) on all tile + 1 frames and cut to the launch: a frame's results depend on its own row only."""
    ref = tr.restrict(full_reference(n_fft, hop, n_mel, None if mut == "skip_last_frame" else mut), frames_of(T), T)
    if mut == "skip_last_frame":
        for b, nf in enumerate(frames_of(T)):
            ref["skipped"][b, min(nf, T) - 1] = True
    return ref


def clip_row_accs(n_fft, hop, n_mel):
    """The restated sums of the clip row on the three constructed frames (host module: must be nextafter(clip, 0), clip, nextafter(clip, inf))."""
    ref = full_reference(n_fft, hop, n_mel)
    return ref["acc"][0, :3, 0], ref["clamped"][0, :3, 0]
