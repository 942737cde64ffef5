"""The conditioning definition of include/e2etts_condition.h in plain Python integers, independent of the kernels and of plan.h: positions,
downmix, rms, detect_silence, the kept span of both trim modes, set_loudness.  tests/test_condition_host.py pins it to audioop (live, and as
recorded in tests/golden/condition_cases.npz); the GPU tests compare the library with it bit for bit."""
import math

import numpy as np

W_DEFAULT, K_DEFAULT = 100, 103   # min_silence_len; floor(10 ** (-50 / 20) * 32768)


def pos(p, rate):
    return p * rate // 1000


def len_ms(n, rate):
    return round(1000 * (n / rate))


def downmix(frames):
    """[n, 2] int16 -> [n] int16: floor(l * 0.5 + r * 0.5)"""
    f = np.asarray(frames, np.int64)
    return np.floor_divide(f[:, 0] + f[:, 1], 2).astype(np.int16)


def _prefix(x):
    c = np.zeros(len(x) + 1, np.int64)   # exact: a row of 2^32 samples sums to 2^62
    np.cumsum(np.asarray(x, np.int64) ** 2, out=c[1:])
    return c


def sumsq(x, a, b):
    """Sum of squares of samples [a, b), zeros past the end, as a Python int."""
    n = len(x)
    c = _prefix(x)
    return int(c[min(b, n)]) - int(c[min(a, n)])


def rms(x, a=0, b=None):
    b = len(x) if b is None else b
    return math.isqrt(sumsq(x, a, b) // (b - a)) if b > a else 0


def silent_starts(x, rate, W=W_DEFAULT, k=K_DEFAULT):
    n, L = len(x), len_ms(len(x), rate)
    if L < W:
        return []
    c = _prefix(x)
    out = []
    for i in range(L - W + 1):
        a, b = pos(i, rate), pos(i + W, rate)
        if int(c[min(b, n)]) - int(c[min(a, n)]) < (k + 1) ** 2 * (b - a):
            out.append(i)
    return out


def ranges_of(starts, W=W_DEFAULT):
    """Walk the silent starts in order: a start more than W after its predecessor opens a new range; [first start, last start + W]."""
    out = []
    prev = None
    for b in starts:
        if prev is None or b > prev + W:
            out.append([b, b + W])
        else:
            out[-1][1] = b + W
        prev = b
    return out


def detect_silence(x, rate, W=W_DEFAULT, k=K_DEFAULT):
    return ranges_of(silent_starts(x, rate, W, k), W)


def kept_span(ranges, L, trim):
    """-> (s_ms, e_ms, sliced).  trim: None | "reference" | "both"."""
    if not ranges or trim is None:
        return 0, L, False
    s = ranges[0][1] if ranges[0][0] == 0 else 0
    e = L   # the reference tests silent[-1][-1] == 0: never true
    if trim == "both" and ranges[-1][1] == L:
        e = ranges[-1][0]
    return s, e, True


def remove_silent(x, rate, trim, W=W_DEFAULT, k=K_DEFAULT):
    """-> (kept samples int16 with the zero padding past the end, s_ms, e_ms, ranges)"""
    x = np.asarray(x, np.int16)
    L = len_ms(len(x), rate)
    rg = detect_silence(x, rate, W, k)
    s, e, sliced = kept_span(rg, L, trim)
    if not sliced:
        return x.copy(), s, e, rg
    a, b = pos(s, rate), pos(e, rate)
    out = np.zeros(max(0, b - a), np.int16)
    src = x[a:b]
    out[:len(src)] = src
    return out, s, e, rg


def dbfs(r):
    return 20 * math.log(r / 32768, 10) if r else -math.inf


def gain_for(x, target):
    r = rms(x)
    return 10 ** ((target - dbfs(r)) / 20) if r else 1.0


def mul(x, gain):
    """audioop.mul on int16: floor(clamp(v * gain)) in double"""
    return np.floor(np.minimum(np.maximum(np.asarray(x, np.float64) * float(gain), -32768.0), 32767.0)).astype(np.int16)


def normalize(x, rate, trim=None, loudness=None, W=W_DEFAULT, k=K_DEFAULT):
    """One mono row -> dict(pcm, n_out, s_ms, e_ms, ranges, gain, sumsq)"""
    kept, s, e, rg = remove_silent(x, rate, trim, W, k)
    g = gain_for(kept, loudness) if loudness is not None else 1.0
    return {"pcm": mul(kept, g), "n_out": len(kept), "s_ms": s, "e_ms": e, "ranges": rg, "gain": g, "sumsq": sumsq(kept, 0, len(kept))}


def batch(rows, width=None, dtype=np.int16):
    """Ragged rows -> ([B, width] zero-padded, lens)"""
    lens = np.array([len(r) for r in rows], np.int64)
    width = int(lens.max()) if width is None else width
    out = np.zeros((len(rows), max(width, 1)), dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, lens
