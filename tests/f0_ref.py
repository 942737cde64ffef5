"""The pitch tracker's definition (include/e2etts_f0.h) in numpy float64, written from the header and independently of the kernels, with
the margin of every discrete decision and the error bars the GPU tests hold the kernels to.  No GPU needed.

Bars (derived, not measured; u = 2^-24, gamma(n) = n u / (1 - n u), in the style of tests/kernel_ref.py).
  a      the kernel rounds m once (a float64 sum, then fp32), then x - m, then the product with w:
         |a32 - a| <= u (|m| w + 2 |a|) =: da.
  r_a    the header fixes the order: chunks of 32 terms in one accumulator (one fused multiply-add per term), the chunk sums added in
         order.  With S[tau] = sum |a[i] a[i + tau]|:  |r_a32 - r_a| <= gamma(32 + ceil(Wp / 32)) S[tau] + sum (da[i] |a[i + tau]| + |a[i]| da[i + tau]) =: dN[tau].
  r      r = r_a[tau] / (r_a[0] r_w[tau]) through one product and one division:  core[tau] = dN[tau] / (r_a[0] r_w[tau]) + 2 u |r[tau]| bounds
         the error against r scaled by the common factor r_a[0] / r_a32[0] (which changes no comparison between lags);
         bar_r[tau] = core[tau] + |r[tau]| dN[0] / r_a[0] bounds the error against r itself.  Both carry a factor 1.001 for the second-order terms.
  f, s   first order in bar_r through the parabola, plus the fp32 evaluation's own roundings (the cancellation in the parabola's
         denominator included).
A decision is compared only where its margin exceeds the bar propagated to it: a local maximum's min(r[tau] - r[tau - 1], r[tau] -
r[tau + 1], r[tau]) against the sum of the two cores involved (times 1 + 1e-4 for the common factor), the K - 1 cut's strength gap against the
two strengths' bars."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.001
CHUNK = 32   # of the header's summation order

DEFAULTS = dict(floor=80.0, ceiling=750.0, voicing_threshold=0.5, silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35,
                voiced_unvoiced_cost=0.14, max_candidates=15)


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def geometry(sr, floor, ceiling):
    W = int(math.floor(3.0 * sr / floor))
    if W % 2 == 0:
        W += 1
    return W, int(math.ceil(sr / ceiling)), int(math.floor(sr / floor))


def tables(sr, floor):
    """(w, r_w) as the kernel is loaded with them: float64 values of the fp32-rounded tables."""
    W, _, tau_max = geometry(sr, floor, 2 * floor)
    i = np.arange(W, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / W)
    rw = np.array([np.dot(w[:W - t], w[t:]) for t in range(tau_max + 2)]) / np.dot(w, w)
    return w.astype(np.float32).astype(np.float64), rw.astype(np.float32).astype(np.float64)


def as_float64(x):
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float32).astype(np.float64)


def frame_windows(x, n, sr, hop, floor):
    """[T, W] float64: the windows of a row of n valid samples (zeros outside [0, n))."""
    W, _, _ = geometry(sr, floor, 2 * floor)
    h = (W - 1) // 2
    T = n // hop
    xp = np.concatenate([np.zeros(h + 1), as_float64(x)[:n], np.zeros(h + hop + 1)])
    c = np.arange(T) * hop + hop // 2
    return np.stack([xp[h + 1 + ci - h: h + 1 + ci + h + 1] for ci in c]) if T else np.zeros((0, W))


def acf(x, n, sr, hop, **params):
    """-> dict of [T, ...] arrays: r [T, NL], bar_r, core, peaks p [T], valid [T] (r_a[0] > 0)."""
    p = {**DEFAULTS, **params}
    W, tau_min, tau_max = geometry(sr, p["floor"], p["ceiling"])
    NL = tau_max + 2
    w, rw = tables(sr, p["floor"])
    win = frame_windows(x, n, sr, hop, p["floor"])
    T = win.shape[0]
    r, bar, core, peaks, valid, means = np.zeros((T, NL)), np.zeros((T, NL)), np.zeros((T, NL)), np.zeros(T), np.zeros(T, bool), np.zeros(T)
    Wp = (W + 3) // 4 * 4
    g_sum = gamma(CHUNK + (Wp + CHUNK - 1) // CHUNK)
    for t in range(T):
        xs = win[t]
        m = means[t] = xs.mean()
        d = xs - m
        peaks[t] = np.abs(d).max()
        a = d * w
        ra = np.correlate(a, a, "full")[W - 1:W - 1 + NL]
        if not ra[0] > 0:
            continue
        valid[t] = True
        aa = np.abs(a)
        da = U * (abs(m) * w + 2 * aa)
        S = np.correlate(aa, aa, "full")[W - 1:W - 1 + NL]
        c1 = np.correlate(da, aa, "full")
        D = c1[W - 1:W - 1 + NL] + c1[W - 1:W - 1 - NL:-1]
        dN = g_sum * S + D
        r[t] = ra / (ra[0] * rw)
        core[t] = SECOND_ORDER * (dN / (ra[0] * rw) + 2 * U * np.abs(r[t]))
        bar[t] = core[t] + SECOND_ORDER * np.abs(r[t]) * dN[0] / ra[0]
    return dict(r=r, bar_r=bar, core=core, peaks=peaks, valid=valid, means=means, T=T, NL=NL, tau_min=tau_min, tau_max=tau_max, W=W)


def candidates(x, n, sr, hop, **params):
    """The voiced candidates of every frame and the unvoiced strength.  -> dict:
      freq, strength [T, K] float64 (index 0 unvoiced; empty slots f = 0, s = -inf), lag [T, K] int (0 in empty slots and at index 0),
      bar_f, bar_s [T, K], frame_ok [T] (every maximum's margin and the K - 1 cut's gap exceed their bars), max_margin / cut_margin [T]
      (the smallest margin of the frame's maxima; the gap at the cut, inf where nothing is cut), n_maxima [T], and acf()'s fields."""
    p = {**DEFAULTS, **params}
    A = acf(x, n, sr, hop, **params)
    T, K = A["T"], int(p["max_candidates"])
    tau_min, tau_max = A["tau_min"], A["tau_max"]
    freq, stren, lag = np.zeros((T, K)), np.full((T, K), -np.inf), np.zeros((T, K), np.int64)
    bar_f, bar_s = np.zeros((T, K)), np.zeros((T, K))
    frame_ok, max_margin, cut_margin, n_max = np.ones(T, bool), np.full(T, np.inf), np.full(T, np.inf), np.zeros(T, np.int64)
    g = A["peaks"].max() if T else 0.0
    vt, st = p["voicing_threshold"], p["silence_threshold"]
    for t in range(T):
        stren[t, 0] = vt + 2.0 if g == 0 else vt + max(0.0, 2.0 - (A["peaks"][t] / g) / (st / (1.0 + vt)))
        if not A["valid"][t]:
            continue
        r, e, core = A["r"][t], A["bar_r"][t], A["core"][t]
        tau = np.arange(tau_min, tau_max + 1)
        rm, r0, rp = r[tau - 1], r[tau], r[tau + 1]
        # every lag's three comparisons as one signed margin (positive = a maximum; for a non-maximum the most negative of the three):
        # the fp32 kernel may decide a lag differently only when |margin| is within the bar, and such a lag fails the frame
        marg = np.minimum(np.minimum(r0 - rm, r0 - rp), r0)
        mbar = (1 + 1e-4) * np.maximum(np.maximum(core[tau] + core[tau - 1], core[tau] + core[tau + 1]), core[tau])
        is_max = (r0 > rm) & (r0 >= rp) & (r0 > 0)
        unsafe = np.abs(marg) <= mbar
        frame_ok[t] = not unsafe.any()
        max_margin[t] = np.abs(marg[is_max]).min() if is_max.any() else np.inf
        n_max[t] = int(is_max.sum())
        taus = tau[is_max]
        rm, r0, rp, em, e0, ep = rm[is_max], r0[is_max], rp[is_max], e[taus - 1], e[taus], e[taus + 1]
        nn, q = rm - rp, rm - 2 * r0 + rp
        d = 0.5 * nn / q
        # first order in the bars, then the fp32 evaluation: nn and q are rounded (q after a cancellation), the quotient once more
        dd = (0.5 * np.abs(q - nn) * em + np.abs(nn) * e0 + 0.5 * np.abs(q + nn) * ep) / q ** 2
        dd += 0.5 * (U * np.abs(nn) / np.abs(q) + np.abs(nn) * U * (np.abs(rm - 2 * r0) + np.abs(q)) / q ** 2) + 2 * U * np.abs(d)
        v_raw = r0 - 0.25 * nn * d
        dv = e0 + 0.25 * np.abs(d) * (em + ep) + 0.25 * np.abs(nn) * dd + 4 * U * (np.abs(r0) + np.abs(0.25 * nn * d))
        v = np.minimum(1.0, v_raw)
        lg = taus + d
        f = sr / lg
        df = sr / lg ** 2 * dd + 4 * U * f
        lg2 = np.log2(p["floor"] * lg / sr)
        s = v - p["octave_cost"] * lg2
        ds = dv + p["octave_cost"] * dd / (lg * math.log(2.0)) + 8 * U * (np.abs(v) + p["octave_cost"] * (np.abs(lg2) + 1.0))
        order = np.lexsort((taus, -s))   # descending strength, a tie to the smaller tau
        keep = order[:K - 1]
        if order.size > K - 1:
            cut_margin[t] = s[order[K - 2]] - s[order[K - 1]]
            if cut_margin[t] <= ds[order[K - 2]] + ds[order[K - 1]]:
                frame_ok[t] = False
        k = keep.size
        freq[t, 1:1 + k], stren[t, 1:1 + k], lag[t, 1:1 + k] = f[keep], s[keep], taus[keep]
        bar_f[t, 1:1 + k], bar_s[t, 1:1 + k] = SECOND_ORDER * df[keep], SECOND_ORDER * ds[keep]
    # the unvoiced strength's bar: p_t and g are fp32 in the kernel, each |x - m32| of one sample (relative error u (1 + |m| / g) at most where
    # it matters); s_u's slope in p / g is 1 / (silence_threshold / (1 + voicing_threshold))
    if T and g > 0:
        rel = 2 * U * (1.0 + np.abs(A["means"]).max() / g)
        bar_s[:, 0] = SECOND_ORDER * (2 * rel * (A["peaks"] / g) / (st / (1.0 + vt)) + 2 * U * stren[:, 0])
    out = dict(A)
    out.update(freq=freq, strength=stren, lag=lag, bar_f=bar_f, bar_s=bar_s, frame_ok=frame_ok, max_margin=max_margin, cut_margin=cut_margin, n_maxima=n_max, g=g)
    return out


def viterbi(freq, strength, sr, hop, **params):
    """The path over one row's candidates [T, K] (float32 or float64 values; strength -inf = empty) in float64.
    -> (f0 [T], index [T], margin): margin = the smallest gap between the best and the second-best predecessor over the cells of the
    chosen path, and between the best and the second-best end cell (inf where there is no second)."""
    p = {**DEFAULTS, **params}
    f, s = np.asarray(freq, np.float64), np.asarray(strength, np.float64)
    T, K = f.shape
    if T == 0:
        return np.zeros(0), np.zeros(0, np.int64), np.inf
    c = 0.01 * sr / hop
    vuc, ojc = p["voiced_unvoiced_cost"] * c, p["octave_jump_cost"] * c
    voiced = (f > 0) & (s > -np.inf)
    lf = np.where(voiced, np.log2(np.where(voiced, f, 1.0)), 0.0)
    delta = np.where(s[0] > -np.inf, s[0], -np.inf)
    bp, gaps = np.zeros((T, K), np.int64), np.full((T, K), np.inf)
    for t in range(1, T):
        vi, vj = voiced[t - 1][:, None], voiced[t][None, :]
        cost = np.where(vi & vj, ojc * np.abs(lf[t - 1][:, None] - lf[t][None, :]), np.where(vi != vj, vuc, 0.0))
        val = delta[:, None] - cost                     # [from, to]
        bp[t] = np.argmax(val, axis=0)                  # the first maximum: the lower index
        best = val.max(axis=0)
        if K > 1:
            srt = np.sort(val, axis=0)
            with np.errstate(invalid="ignore"):
                gaps[t] = np.where(np.isfinite(srt[-2]), srt[-1] - srt[-2], np.inf)
        delta = np.where(s[t] > -np.inf, best + s[t], -np.inf)
    j = int(np.argmax(delta))
    fin = np.sort(delta[np.isfinite(delta)])
    margin = fin[-1] - fin[-2] if fin.size > 1 else np.inf
    idx = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        idx[t] = j
        if t > 0:
            margin = min(margin, gaps[t, j])
            j = int(bp[t, j])
    return f[np.arange(T), idx], idx, float(margin)


def track(x, n, sr, hop, **params):
    """The whole definition for one row.  -> dict: f0 [T], index [T], path_margin, path_budget (twice the sum over the frames of the largest
    strength bar plus the transition costs' own: a path gap above it cannot be closed by the kernel's fp32 candidates), and candidates()'s fields."""
    p = {**DEFAULTS, **params}
    C = candidates(x, n, sr, hop, **params)
    f0, idx, margin = viterbi(C["freq"], C["strength"], sr, hop, **params)
    c = 0.01 * sr / hop
    with np.errstate(divide="ignore", invalid="ignore"):
        dlog = np.where(C["freq"] > 0, C["bar_f"] / (C["freq"] * math.log(2.0)), 0.0)
    per_frame = C["bar_s"].max(axis=1) + 2 * p["octave_jump_cost"] * c * dlog.max(axis=1) if C["T"] else np.zeros(0)
    out = dict(C)
    out.update(f0=f0, index=idx, path_margin=margin, path_budget=2.0 * float(per_frame.sum()))
    return out


def targets(f0_hz, mean=None, std=None, mode="linear", eps=1e-9):
    """get_f0 for one row [T] in float64, written out (np.interp's arithmetic spelled: slope = (y1 - y0) / (x1 - x0), slope (x - x0) + y0).
    -> (f0 target float64, uv float32)."""
    f0 = np.asarray(f0_hz, np.float64)
    uv = f0 == 0
    y = np.log2(f0 + eps) if mode == "log" else (f0 - mean) / std
    vi = np.flatnonzero(~uv)
    out = y.copy()
    if vi.size == 0:
        out[:] = 0.0
    else:
        for t in np.flatnonzero(uv):
            k = np.searchsorted(vi, t)
            if k == 0:
                out[t] = y[vi[0]]
            elif k == vi.size:
                out[t] = y[vi[-1]]
            else:
                x0, x1 = vi[k - 1], vi[k]
                slope = (y[x1] - y[x0]) / float(x1 - x0)
                out[t] = slope * float(t - x0) + y[x0]
    return out, uv.astype(np.float32)
