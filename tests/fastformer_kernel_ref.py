"""Restatement of csrc/fastformer.hip one launch at a time (launch_ff_pool, launch_ff_scale), for tests/test_gpu_fastformer_kernels.py and
tests/test_fastformer_kernel_ref_host.py.

What is restated exactly (float32, one rounding per written operation, bit for bit):
  ff_shape    the launch shape: RP, threads, rows per workgroup (a "run"), splits, LDS bytes -- a restatement of fastformer.hip's ff_shape();
  logits_f32  s[n] = fl(fl(fl(chain + bias) / div) + shift), chain = the fmaf chain over all H channels in ascending k from +0 (an EXACT fused
              multiply-add, see fma32), the second pool's v * scale rounded once before the chain, div = fl32(sqrt(head_size)), shift = -10000
              at n < clamp(lens[b], 0, N) and 0 elsewhere (the reference's inverted mask);
  scale_f32   ff_scale's two outputs.
What is restated in float64 as the reference: pool64, the softmax-weighted sum over the restated logits (float32 values, taken as given).
What is restated in float32 as a YARDSTICK, not bit for bit (numpy's expf is not the device's): pool_f32, in the kernel's own order.

The bar of pool64 (per output element, first order in U = 2^-24, everything relative to S = sum_n w_n |v_n| with w the float64 softmax):
  * The weight of row n reaches the output as a product of exponentials: expf(s_n - m) inside its tile, expf(m - m') at every later tile
    of its run (the online rescale), expf(m_run - M) in the merge.  The maxima only rise, so the arguments' magnitudes add up to
    exactly |s_n - M|; each difference is rounded once (U relative on the argument = U |argument| relative on the exponential), which
    gives U |s_n - M| in all.  Each expf is K ulp = 2 K U off (K = 4, tests/small_ref.py's allowance: ASSUMED, NOT MEASURED); there are at
    most tiles_per_run + 1 of them on a row's path (its own, tiles_per_run - 1 rescales, the merge).  eps_n = U |s_n - M| + 2 K U
    (tiles_per_run + 1).  The numerator carries sum_n w_n |v_n| eps_n, the denominator sum_n w_n eps_n relative, i.e. at most S sum_n w_n eps_n
    on the quotient.
  * Accumulation: on an element's path lie rows_per_run fused accumulations, tiles_per_run rescaling products, `runs` fused accumulations
    in the merge, for the numerator and again for the denominator (all its terms positive), and one division:
    (2 (rows_per_run + tiles_per_run + runs) + 1) U S.
  * Weights below 2^-126: an expf result in the subnormals (or flushed) is off by at most 2^-126 absolutely; the denominator is at least 1
    after the merge (the row that holds the maximum), so N 2^-126 max|v| covers them.
  bar = SECOND_ORDER x (the three above) + 2^-149.  Nothing in it was fitted to an output.
Aggregate rule, as elsewhere: for cases of at least AGG_MIN_ELEMS output elements the kernel's mean |deviation| from pool64 is at most
AGG_FACTOR x that of pool_f32."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from aligner_ref import K_ULP, SECOND_ORDER, U

f32, f64 = np.float32, np.float64
FF_MAX_THREADS, FF_MAX_HEADS, FF_TARGET_WG, FF_MAX_LDS, TILE = 1024, 512, 1024, 65536, 16
AGG_MIN_ELEMS, AGG_FACTOR = 512, 4.0
SHIFT = f32(-10000.0)
FMA_STATS = {"rational": 0}   # elements fma32 has re-evaluated in rational arithmetic (the host test asserts that its constructed ties get there)


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def diff_count(a, b) -> int:
    """Elements whose bits differ (two NaNs count as equal)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.count_nonzero((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------- an exact float32 fused multiply-add
def round_fraction_f32(x: Fraction) -> np.float32:
    """A rational number rounded once to float32, to nearest, ties to even (subnormals included; no overflow handling: |x| < 2^128)."""
    if x == 0:
        return f32(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)
    t = a / q
    n = t.numerator // t.denominator
    r = t - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    v = float(n * q)          # exact in float64: n < 2^25
    return f32(-v if x < 0 else v)


def fma_fraction(a, b, c) -> np.float32:
    """fmaf(a, b, c) in rational arithmetic: the definition fma32 is checked against."""
    return round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly.  The product of two float32 is exact in float64; the float64 sum p + c is rounded once more
    when it goes to float32, which is wrong only where that sum was INEXACT and its rounded value lies exactly on a float32 tie -- those
    elements (found with the error term of the exact two-sum) are evaluated again in rational arithmetic.  Finite operands, no overflow."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p = a.astype(f64) * b.astype(f64)
    c64 = c.astype(f64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)       # two-sum: p + c = s + err exactly
    r = s.astype(f32)
    r64 = r.astype(f64)
    off = (r64 != s) & (err != 0)
    if np.any(off):
        idx = np.flatnonzero(off)
        rf, sf = r.reshape(-1)[idx], s.reshape(-1)[idx]
        nb = np.nextafter(rf, np.where(sf > rf.astype(f64), f32(np.inf), f32(-np.inf)).astype(f32))
        tie = (rf.astype(f64) + nb.astype(f64)) * 0.5 == sf
        if np.any(tie):
            r = r.copy()
            flat = r.reshape(-1)
            af, bf, cf = a.reshape(-1), b.reshape(-1), c.reshape(-1)
            for i in idx[tie]:
                flat[i] = fma_fraction(af[i], bf[i], cf[i])
            FMA_STATS["rational"] += int(tie.sum())
    return r


def fma32_once(a, b, c):
    """The float64 shortcut fl32(fl64(a * b + c)): what the yardstick accumulates with (it double-rounds on rare ties; the yardstick is not
    compared bit for bit)."""
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


# ---------------------------------------------------------------- the launch shape
def ff_check(B, N, H, hs):
    """launch_ff_pool's message for the dimensions, None when it takes them."""
    if B <= 0 or B > 65535 or N <= 0 or N > (1 << 24):
        return "ff_pool: bad batch / sequence size"
    if H <= 0 or H > 1024 or (H & 3):
        return "ff_pool: hidden must be a multiple of 4 in (0, 1024]"
    if hs not in (1, 2, 4, 8):
        return "ff_pool: head size must be 1, 2, 4 or 8"
    if H % hs or H // hs > FF_MAX_HEADS:
        return "ff_pool: hidden / head size must be an integer of at most 512"
    return None


def ff_shape(B, N, H, hs):
    """dict(rp, maxt, threads, rows_per_wg, splits, lds, heads, tiles_per_run): which of the five instantiations of ff_pool_partial_kernel a
    launch takes (rp 4 / 2 / 1; maxt = the workgroup size it is compiled for, 1024 above 512 threads) and how the rows are split."""
    assert ff_check(B, N, H, hs) is None
    NH = H // hs

    def fits(rp):
        if NH * rp > FF_MAX_THREADS:
            return None
        threads = (NH * rp + 63) // 64 * 64
        lds = (TILE * H + (TILE * NH if rp > 1 else 0)) * 4
        return dict(rp=rp, threads=threads, lds=lds) if lds <= FF_MAX_LDS else None

    small = B * N < 8192
    s = (fits(4) if small else None) or fits(2) or fits(1)
    assert s is not None
    tiles_n = (N + TILE - 1) // TILE
    per = max(1, (B * tiles_n + FF_TARGET_WG - 1) // FF_TARGET_WG)
    s["rows_per_wg"] = min(per * TILE, tiles_n * TILE)
    s["splits"] = (N + s["rows_per_wg"] - 1) // s["rows_per_wg"]
    s["maxt"] = 1024 if s["threads"] > 512 else 512
    if s["rp"] == 1:
        s["maxt"] = 512
    s["heads"] = NH
    s["tiles_per_run"] = s["rows_per_wg"] // TILE
    return s


def workspace_bytes(B, N, H, hs) -> int:
    return 0 if ff_check(B, N, H, hs) else B * ff_shape(B, N, H, hs)["splits"] * (H // hs) * (hs + 2) * 4


def run_bounds(N, sh):
    return [(sp * sh["rows_per_wg"], min(N, (sp + 1) * sh["rows_per_wg"])) for sp in range(sh["splits"])]


# ---------------------------------------------------------------- the logits
def clamp_lens(lens, B, N):
    return np.full(B, N, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, N)


def scaled_values(v, scale):
    """v' = fl(v * scale[b, :]) (one rounding), or v."""
    v = np.asarray(v, f32)
    return v if scale is None else (v * np.asarray(scale, f32)[:, None, :]).astype(f32)


def chain_f32(vp, wl_t, mut=None):
    """[B, N, H] . [H, heads] -> [B, N, heads]: per element ONE fmaf chain over k = 0 .. H - 1 from +0.
    mut: "drop_last_group" (the chain stops four channels early), "ksplit4" (four chains over the four contiguous quarters of K, added
    pairwise afterwards)."""
    vp, wl_t = np.asarray(vp, f32), np.asarray(wl_t, f32)
    B, N, H = vp.shape
    NH = wl_t.shape[1]

    def chain(k0, k1):
        acc = np.zeros((B, N, NH), f32)
        for k in range(k0, k1):
            acc = fma32(vp[:, :, k, None], wl_t[None, None, k, :], acc)
        return acc

    if mut == "drop_last_group":
        return chain(0, H - 4)
    if mut == "ksplit4":
        q = H // 4
        p = [chain(j * q, (j + 1) * q) for j in range(4)]
        return ((p[0] + p[1]).astype(f32) + (p[2] + p[3]).astype(f32)).astype(f32)
    return chain(0, H)


def logits_f32(v, scale, wl_t, bl, lens, hs, mut=None):
    """s [B, heads, N] float32, bit for bit what ff_pool_partial_kernel feeds its softmax.
    mut: None | "mask_not_inverted" | "mask_off_by_one" | "div_after_shift" | "scale_not_in_logits" | chain_f32's."""
    v = np.asarray(v, f32)
    B, N, H = v.shape
    vp = scaled_values(v, None if mut == "scale_not_in_logits" else scale)
    ch = chain_f32(vp, wl_t, mut)
    div = f32(np.sqrt(f64(hs)))
    len_ = clamp_lens(lens, B, N)
    n = np.arange(N)[None, :]
    if mut == "mask_not_inverted":
        valid = n >= len_[:, None]
    elif mut == "mask_off_by_one":
        valid = n <= len_[:, None]
    else:
        valid = n < len_[:, None]
    shift = np.where(valid, SHIFT, f32(0.0)).astype(f32)[:, :, None]
    t = (ch + np.asarray(bl, f32)[None, None, :]).astype(f32)
    if mut == "div_after_shift":
        s = ((t + shift).astype(f32) / div).astype(f32)
    else:
        s = ((t / div).astype(f32) + shift).astype(f32)
    return np.ascontiguousarray(s.transpose(0, 2, 1))


def exp_facts():
    """What the exact tier rests on, for float32 exponentials of any sane implementation: asserted on numpy's."""
    with np.errstate(under="ignore"):
        assert np.exp(f32(0.0)) == f32(1.0)
        for x in (-10000.0, -9990.0, -10010.0, -200.0, -104.0):
            assert np.exp(f32(x)) == f32(0.0), x
        assert np.exp(f32(-np.inf)) == f32(0.0)


# ---------------------------------------------------------------- the pool
def pool64(s, vp, hs):
    """out [B, H] float64 = sum_n softmax_n(s[b, h, :]) vp[b, n, h hs + d]; also S = sum_n w_n |vp| and the weights w [B, heads, N]."""
    s64, v64 = np.asarray(s, f32).astype(f64), np.asarray(vp, f32).astype(f64)
    B, NH, N = s64.shape
    e = np.exp(s64 - s64.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    vh = v64.reshape(B, N, NH, hs)
    out = np.einsum("bhn,bnhd->bhd", w, vh).reshape(B, NH * hs)
    S = np.einsum("bhn,bnhd->bhd", w, np.abs(vh)).reshape(B, NH * hs)
    return out, S, w


def pool_bar(s, vp, hs, sh):
    """The derived bar of the module's docstring, [B, H]."""
    s64, v64 = np.asarray(s, f32).astype(f64), np.asarray(vp, f32).astype(f64)
    B, NH, N = s64.shape
    _, S, w = pool64(s, vp, hs)
    eps = U * np.abs(s64 - s64.max(-1, keepdims=True)) + 2 * K_ULP * U * (sh["tiles_per_run"] + 1)
    eps = np.where(w > 0, eps, 0.0)                      # (a weight that is exactly 0 in float64 carries nothing; |s - M| may be 1e4 there)
    av = np.abs(v64.reshape(B, N, NH, hs))
    num = np.einsum("bhn,bnhd->bhd", w * eps, av).reshape(B, NH * hs)
    den = (w * eps).sum(-1)[:, :, None].repeat(hs, 2).reshape(B, NH * hs) * S
    ops = 2 * (min(sh["rows_per_wg"], N) + sh["tiles_per_run"] + sh["splits"]) + 1
    tiny = N * 2.0 ** -126 * float(np.abs(v64).max())
    return SECOND_ORDER * (num + den + ops * U * S + tiny) + 2.0 ** -149


def _exp32(x):
    with np.errstate(under="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, f32)).astype(f32)


def pool_f32(s, vp, hs, sh, mut=None, zero_logit=None):
    """(out [B, H], ws [B, splits, heads, hs + 2]) in float32 in the kernel's own order: tiles of 16 rows in row order, a running (max, sum,
    weighted sums) with the rescale between tiles, runs of rows_per_wg rows, the merge in run order with fused accumulations, the division.
    mut: None | "no_rescale" | "merge_without_maxima" | "drop_last_run" | "head_plus_one" (head h accumulates slice h + 1) | "stale_rows":
    the rows a partial tile does not have take part as the zero rows the staging left there, with zero_logit [heads], the logit of a zero
    row at a padded position (a partial tile is the last of the sequence: its missing rows lie past N)."""
    s, vp = np.asarray(s, f32), np.asarray(vp, f32)
    B, NH, N = s.shape
    vh = vp.reshape(B, N, NH, hs)
    if mut == "head_plus_one":
        vh = np.roll(vh, -1, axis=2)
    ws = np.zeros((B, sh["splits"], NH, hs + 2), f32)
    with np.errstate(invalid="ignore", under="ignore"):
        for sp, (n_begin, n_end) in enumerate(run_bounds(N, sh)):
            m = np.full((B, NH), -np.inf, f32)
            l = np.zeros((B, NH), f32)
            a = np.zeros((B, NH, hs), f32)
            for n0 in range(n_begin, n_end, TILE):
                n1 = min(n0 + TILE, n_end)
                lg = s[:, :, n0:n1]
                vt = vh[:, n0:n1]
                if mut == "stale_rows" and n1 - n0 < TILE:
                    extra = TILE - (n1 - n0)
                    lg = np.concatenate([lg, np.broadcast_to(np.asarray(zero_logit, f32)[None, :, None], (B, NH, extra))], 2)
                    vt = np.concatenate([vt, np.zeros((B, extra, NH, hs), f32)], 1)
                mn = np.maximum(m, lg.max(-1))
                sc = _exp32(m - mn) if mut != "no_rescale" or n0 == n_begin else np.ones_like(m)
                l = (l * sc).astype(f32)
                a = (a * sc[:, :, None]).astype(f32)
                for r in range(lg.shape[2]):
                    p = _exp32(lg[:, :, r] - mn)
                    l = (l + p).astype(f32)
                    a = fma32_once(p[:, :, None], vt[:, r], a)
                m = mn
            ws[:, sp, :, 0], ws[:, sp, :, 1], ws[:, sp, :, 2:] = m, l, a
        return merge_f32(ws, mut), ws


def merge_f32(ws, mut=None):
    """ff_pool_merge_kernel on a workspace: out [B, heads * hs]."""
    ws = np.asarray(ws, f32)
    B, splits, NH, w2 = ws.shape
    if mut == "drop_last_run" and splits > 1:
        splits -= 1
    M = ws[:, :splits, :, 0].max(1)
    L = np.zeros((B, NH), f32)
    A = np.zeros((B, NH, w2 - 2), f32)
    with np.errstate(invalid="ignore", under="ignore"):
        for sp in range(splits):
            w = np.ones((B, NH), f32) if mut == "merge_without_maxima" else _exp32(ws[:, sp, :, 0] - M)
            L = fma32_once(ws[:, sp, :, 1], w, L)
            A = fma32_once(ws[:, sp, :, 2:], w[:, :, None], A)
        return (A / L[:, :, None]).astype(f32).reshape(B, NH * (w2 - 2))


def run_maxima(s, N, sh):
    """[B, splits, heads]: the largest restated logit of every run -- what the workspace's first entry must equal bit for bit."""
    return np.stack([np.asarray(s, f32)[:, :, a:b].max(-1) for a, b in run_bounds(N, sh)], 1)


# ---------------------------------------------------------------- ff_scale
def scale_f32(q, gk, x):
    """(wv, qx): wv[b, n, :] = fl(gk[b, :] * q[b, n, :]), qx = fl(q + x); q, x [B, N, H], gk [B, H]."""
    q, gk, x = np.asarray(q, f32), np.asarray(gk, f32), np.asarray(x, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (gk[:, None, :] * q).astype(f32), (q + x).astype(f32)
