"""The arithmetic of include/e2etts_resample.h restated in numpy, for the resampler's tests: the float64 definition, the derived per-sample
error bar, a float32 emulation of the FMA chain, the listed mistakes, and the stream bookkeeping of csrc/resample/plan.h.

    n_out = ceil(n_valid L / M),  c(m) = m M + half,  y[m] = sum_k x[k] h[c(m) - k L]   (0 <= k < n_valid, 0 <= c(m) - k L <= 2 half)
"""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32

MUTATIONS = ["phase_plus", "phase_minus", "column_off", "first_tap_dropped", "last_tap_dropped", "half_plus", "half_minus", "x_plus", "x_minus"]


def ceil_div(a, b):
    return -((-a) // b)


def n_out(n, L, M):
    return int(ceil_div(int(n) * int(L), int(M)))


def taps_per_output(n_taps, L):
    return int(ceil_div(int(n_taps), int(L)))


def table(taps, L):
    """G[r][i] = h[r + i L], zero past the last tap (float64 values of the fp32 taps)."""
    h = np.asarray(taps, np.float64).reshape(-1)
    P = taps_per_output(h.size, L)
    g = np.zeros(L * P)
    g[:h.size] = h
    return g.reshape(P, L).T.copy()


def _terms(x, taps, L, M, n_valid, ms, mut=None):
    """(X, G) [len(ms), P] float64, columns in the order the chain adds them (k ascending): output m is sum_j X[m, j] * G[m, j]."""
    x = np.asarray(x)
    h = np.asarray(taps, np.float32).astype(np.float64).reshape(-1)
    half = (h.size - 1) // 2 + {"half_plus": 1, "half_minus": -1}.get(mut, 0)
    g = table(h, L)
    P = g.shape[1]
    ms = np.asarray(ms, np.int64)
    c = ms * M + half
    r = c % L
    khi = c // L
    if mut == "phase_plus":
        r = (r + 1) % L
    if mut == "phase_minus":
        r = (r - 1) % L
    i = np.arange(P - 1, -1, -1, dtype=np.int64)   # k = khi - i ascending
    k = khi[:, None] - i[None, :] + {"x_plus": 1, "x_minus": -1}.get(mut, 0)
    ok = (k >= 0) & (k < int(n_valid))
    xf = x.astype(np.float64) / (32768.0 if x.dtype == np.int16 else 1.0)
    X = np.where(ok, xf[np.clip(k, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
    col = i + 1 if mut == "column_off" else i
    G = np.where(col[None, :] < P, g[r[:, None], np.minimum(col, P - 1)[None, :]], 0.0)
    if mut == "first_tap_dropped":    # the chain stops one term early: the phase's first tap h[r] (i = 0, the last k) is missing
        G[:, -1] = 0.0
    if mut == "last_tap_dropped":     # the chain starts one term late: the phase's last tap h[r + i L] (the first k) is missing
        last_i = (2 * half - r) // L
        G[np.arange(ms.size), P - 1 - last_i] = 0.0
    return X, G


def _blocks(n, step=8192):
    for a in range(0, n, step):
        yield a, min(n, a + step)


def resample_f64(x, taps, L, M, n_valid=None, ms=None, mut=None):
    """The definition in float64 on the fp32-rounded taps and inputs (float32, or int16 / 32768): all n_out outputs, or those named in ms."""
    x = np.asarray(x).reshape(-1)
    nv = x.size if n_valid is None else int(n_valid)
    ms = np.arange(n_out(nv, L, M), dtype=np.int64) if ms is None else np.asarray(ms, np.int64)
    y = np.zeros(ms.size)
    for a, b in _blocks(ms.size):
        X, G = _terms(x, taps, L, M, nv, ms[a:b], mut)
        y[a:b] = (X * G).sum(1)
    return y


def bar(x, taps, L, M, n_valid=None, ms=None):
    """(P + 2) 2^-24 sum_k |x[k] h[c - k L]| per output sample: gamma_P = P u / (1 - P u) of a P-term recursive FMA sum (one rounding per
    term), derived rather than measured; the + 2 covers the first-order truncation of gamma for P <= 1024."""
    x = np.asarray(x).reshape(-1)
    nv = x.size if n_valid is None else int(n_valid)
    ms = np.arange(n_out(nv, L, M), dtype=np.int64) if ms is None else np.asarray(ms, np.int64)
    P = taps_per_output(np.asarray(taps).size, L)
    out = np.zeros(ms.size)
    for a, b in _blocks(ms.size):
        X, G = _terms(x, taps, L, M, nv, ms[a:b])
        out[a:b] = np.abs(X * G).sum(1)
    return (P + 2) * U * out


def resample_f32(x, taps, L, M, n_valid=None, ms=None, mut=None):
    """The chain as the kernel runs it: acc = fmaf(x[k], h[..], acc) from +0, k ascending.  The product of two fp32 numbers is exact in
    float64; the sum is rounded to float64 and then to fp32 (a double rounding that differs from a true FMA in rare last-bit cases)."""
    x = np.asarray(x).reshape(-1)
    nv = x.size if n_valid is None else int(n_valid)
    ms = np.arange(n_out(nv, L, M), dtype=np.int64) if ms is None else np.asarray(ms, np.int64)
    y = np.zeros(ms.size, np.float32)
    for a, b in _blocks(ms.size):
        X, G = _terms(x, taps, L, M, nv, ms[a:b], mut)
        acc = np.zeros(b - a, np.float32)
        for j in range(X.shape[1]):
            acc = (X[:, j] * G[:, j] + acc.astype(np.float64)).astype(np.float32)
        y[a:b] = acc
    return y


def pcm_of(y):
    """saturate(trunc(y * 32768)) of fp32 samples (e2etts_denoise's rule)."""
    s = np.trunc(np.asarray(y, np.float32) * np.float32(32768.0))
    return np.clip(s, -32768.0, 32767.0).astype(np.int16)


def failing_fraction(y, ref, tol):
    """Share of samples outside their bar; lengths must agree (a wrong length fails outright: 1.0)."""
    if len(y) != len(ref):
        return 1.0
    return float((np.abs(np.asarray(y, np.float64) - ref) > tol).mean()) if len(ref) else 0.0


# ---- the stream bookkeeping of csrc/resample/plan.h, restated
def emitted(N, L, M, half, last=False):
    if last:
        return n_out(N, L, M)
    return max(0, (N * L - 1 - half) // M + 1)


def history_start(E, L, M, half):
    return max(0, ceil_div(E * M - half, L))


def k_lo(m, L, M, half):
    return ceil_div(m * M + half - 2 * half, L)


def k_hi(m, L, M, half):
    return (m * M + half) // L


def make_signal(n, seed=0, dtype=np.float32):
    """Broadband noise plus two tones, |x| < 1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n, dtype=np.float64)
    x = 0.45 * rng.uniform(-1.0, 1.0, n) + 0.3 * np.sin(0.05 * t) + 0.2 * np.sin(1.3 * t + 0.4)
    if dtype == np.int16:
        return np.round(x * 32767.0).astype(np.int16)
    return x.astype(np.float32)
