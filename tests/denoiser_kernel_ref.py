"""The seven passes of csrc/denoiser.hip restated in numpy float32, ONE rounding per written operation (the contract of csrc/kernels.h), for
the bit-for-bit comparison of tests/test_gpu_denoiser_kernels.py:

    mag = sqrt(fl(fl(re * re) + fl(im * im)));  md = fmax(fl(mag - fl(bias * strength)), 0);  sc = mag > 0 ? fl(md / mag) : 0
    out = fl(re * sc), fl(im * sc)
    env = the float32 accumulator that takes the float64 squared-window term of every covering frame in ascending frame order
    v   = env > FLT_MIN ? fl(v / env) : v, then fl(v * fl(filter_length / hop));  pcm = (int16) fmin(fmax(trunc(fl(v * 32768)), -32768), 32767)

numpy's float32 `*`, `+`, `-`, `/` and `sqrt` are single correctly rounded IEEE operations (subnormals kept), `np.fmax` / `np.fmin` return
the other operand for a NaN as fmaxf / fminf do.  Positions and frame indices are Python integers, so nothing here can wrap at 2^31 or 2^63.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
FLT_MIN = np.finfo(f32).tiny
LLONG_MAX = 2 ** 63 - 1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def diff_count(got, want) -> int:
    """Elements whose bits differ; two NaNs count as equal whatever their payloads."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ne = bits(got) != bits(want)
    if got.dtype.kind == "f":
        ne &= ~(np.isnan(got) & np.isnan(want))
    return int(ne.sum())


# ---------------------------------------------------------------- reflect-pad
def stft_pad_ref(wav, n_valid, R, N, hop):
    """wav [B, >= n_valid[b]] -> [B, R * hop]: half reflected | the row | half reflected at the row's own end | zeros; a row of at most half
    samples: all zeros."""
    half = N // 2
    out = np.zeros((len(n_valid), R * hop), f32)
    for b, nb in enumerate(int(v) for v in n_valid):
        if nb > half:
            assert nb + N <= R * hop
            out[b, :nb + N] = np.pad(np.asarray(wav[b][:nb], f32), half, mode="reflect")
    return out


def stft_pad_stream_ref(seg, L, N, hop, left_real, right_real):
    """seg [B, >= L] -> [B, L + half per real edge]: a real edge reflected, a context edge copied plainly."""
    half = N // 2
    rows = []
    for w in seg:
        w = np.asarray(w[:L], f32)
        rows.append(np.pad(w, (half if left_real else 0, half if right_real else 0), mode="reflect"))
    out = np.stack(rows)
    assert out.shape[1] % hop == 0
    return out


# ---------------------------------------------------------------- spectral subtraction
def magnitude_ref(re, im):
    re, im = np.asarray(re, f32), np.asarray(im, f32)
    with np.errstate(all="ignore"):
        return np.sqrt(re * re + im * im)


def subtract_row_ref(re, im, bias, strength, contract=False):
    """One spectrum row.  contract = True: the mutation the test exists for, mag - bias * strength as ONE fused multiply-add."""
    re, im, bias = np.asarray(re, f32), np.asarray(im, f32), np.asarray(bias, f32)
    with np.errstate(all="ignore"):
        mag = magnitude_ref(re, im)
        if contract:
            d = (mag.astype(np.float64) - bias.astype(np.float64) * np.float64(f32(strength))).astype(f32)   # the product of two float32 is exact in float64
        else:
            d = mag - bias * f32(strength)
        md = np.fmax(d, f32(0))
        sc = np.where(mag > 0, md / mag, f32(0)).astype(f32)
        return re * sc, im * sc, mag, md


def spectral_subtract_ref(spec, bias, frames, N, n_overlap, strength, contract=False):
    """spec [B, R, Cpad] -> the buffer after the launch (rows f < frames[b] subtracted with zeroed padding channels, the next n_overlap - 1
    rows zero, later rows as they were)."""
    B, R, Cpad = spec.shape
    bins = N // 2 + 1
    out = np.array(spec, f32)
    for b in range(B):
        Fb = int(frames[b])
        for f in range(min(Fb, R)):
            re, im, _, _ = subtract_row_ref(spec[b, f, :bins], spec[b, f, bins:2 * bins], bias, strength, contract)
            out[b, f, :bins], out[b, f, bins:2 * bins], out[b, f, 2 * bins:] = re, im, 0
        out[b, Fb:min(Fb + n_overlap - 1, R)] = 0
    return out


# ---------------------------------------------------------------- overlap-add normalisation
def env_at(win_sq, p: int, F: int, hop: int) -> np.float32:
    """The window sum-square envelope at padded position p of a signal of F frames: frames f_lo .. f_hi in ascending order into a float32
    accumulator, each term added in float64 (denoiser_ref.envelope, one position at a time, in Python integers)."""
    N = len(win_sq)
    f_lo = 0 if p - N + 1 <= 0 else (p - N + hop) // hop
    f_hi = min(p // hop, F - 1)
    env = f32(0)
    for f in range(f_lo, f_hi + 1):
        env = f32(np.float64(env) + win_sq[p - f * hop])
    return env


def norm_ref(v, env, N, hop):
    v = f32(v)
    with np.errstate(all="ignore"):
        if env > FLT_MIN:
            v = v / env
        return v * (f32(N) / f32(hop))


def ola_norm_ref(y, inp, n_valid, frames, win_sq, n, N, hop):
    """y [B, R * hop], inp [B, >= n] -> wav [B, n]."""
    half = N // 2
    out = np.zeros((len(n_valid), n), f32)
    for b, nb in enumerate(int(v) for v in n_valid):
        for i in range(min(n, nb)):
            out[b, i] = inp[b][i] if nb <= half else norm_ref(y[b][i + half], env_at(win_sq, i + half, int(frames[b]), hop), N, hop)
    return out


def ola_norm_stream_ref(y, y_off, inp, win_sq, n, p_abs0, F_abs, N, hop, pass_):
    """y [B, y_bs], inp [B, >= n] -> wav [B, n]; sample k sits at absolute padded position p_abs0 + k."""
    B = len(inp) if pass_ else len(y)
    out = np.zeros((B, n), f32)
    for b in range(B):
        for i in range(n):
            out[b, i] = inp[b][i] if pass_ else norm_ref(y[b][y_off + i], env_at(win_sq, p_abs0 + i, F_abs, hop), N, hop)
    return out


def pcm_ref(wav):
    with np.errstate(all="ignore"):
        s = np.trunc(np.asarray(wav, f32) * f32(32768))
        return np.fmin(np.fmax(s, f32(-32768)), f32(32767)).astype(np.int32).astype(np.int16)
