"""numpy float64 references of the operations csrc/kernels.h states, the error bars the kernel tests hold the kernels to, and float32
numpy evaluations of the same operand models (the yardstick of the aggregate bars, and what the mutation tests of
tests/test_kernel_ref_host.py corrupt).  Written from kernels.h and the kernels' own order of terms; no GPU needed.

Operand model.  fp32 (x3 = 0): the operands as they are.  bf16x3 (x3 = 1): every operand v is hi + lo, hi = bf16(v) and lo = bf16(v - hi),
both round-to-nearest-even (split4 in conv_gemm.hip, packer.pack_x3), and the kernel issues lo_a * hi_w, hi_a * lo_w, hi_a * hi_w per term
(three bf16 MFMAs; lo * lo is dropped).  Plain bf16 (x3 = 2, conv_bf16): hi_a * hi_w alone.  The input activation max(x, x * in_slope) is
formed in fp32 BEFORE the split, where the kernel forms it.  The reference sums exactly those products in float64.

Bars.  Per element |got - ref| <= gamma_n * S: S the sum of |terms| of that element (bias, residual and out_old included), n the number
of terms plus the epilogue operations, gamma_n = n u / (1 - n u), u = 2^-24: the worst-case bound of fp32 summation in ANY order (Higham,
Accuracy and Stability of Numerical Algorithms, section 4.2), derived and not measured.  That bar is loose by about sqrt(n), so a second one
bounds the root mean square of err / S over a launch by 4 x the same statistic of a float32 numpy evaluation of the same operand model,
blocked in K by 32 as the kernel chunks: the factor 4 is a margin over that evaluation's own error for a differing summation order, never
over the kernel's.  Where this departs from "one aggregate bar per launch": it is applied to launches of at least AGG_MIN_ELEMS elements (an
RMS over a handful of elements is noise: with 4 elements a correct result misses a factor 4 by chance); launches with a tanh / swish / GELU
epilogue carry it on the same launch with the activation switched off; and the yardstick's statistic is taken on the first utterances of
a launch, YARD_MAX_ROWS rows at most (it is a property of the operand model and the data's distribution, which every utterance shares).

16-bit activations (precisions "bf16_act" / "fp16_act"; the last section).  A 16-bit output leaves no room for such bars -- gamma_n S is a
sizeable part of a bf16 ulp at realistic K and more than an fp16 ulp -- so these kernels are judged in two tiers.  Exact tier: inputs from
dyadic grids whose partial sums are all exactly representable in float32 (act16_exactness states the precondition), so the output must
equal a16_exact() bit for bit.  General tier: Gaussian data under an interval rule (the epilogue is monotone: chain(ref - bar) <= out <=
chain(ref + bar), no element excluded) and an aggregate rule (the share of elements whose bits differ from chain(fl32(ref)) against the
same share of the float32 yardstick)."""
from __future__ import annotations

import zlib

import numpy as np

from kernel_cases import ACT_GELU, ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH

U = 2.0 ** -24
AGG_FACTOR = 4.0
AGG_MIN_ELEMS = 512
# Lipschitz constants of the transcendental epilogues: tanh' <= 1; swish' = s + v s (1 - s) <= 1.0999; gelu' = Phi + v phi <= 1.1290
LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_LRELU: 1.0, ACT_TANH: 1.0, ACT_SWISH: 1.1, ACT_GELU: 1.13}
TRANSCENDENTAL = (ACT_TANH, ACT_SWISH, ACT_GELU)


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def rng_of(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------- bf16 splitting
def bf16_round(x) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.view(np.float32)


def bf16_trunc(x) -> np.ndarray:
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def split_bf16(x, lo_round=bf16_round):
    """(hi, lo) of a float32 array, as float32: hi = bf16(x), lo = bf16(x - hi)."""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_round(x)
    return hi, lo_round(x - hi)


# ---------------------------------------------------------------- activations
def _erf64(x):
    from math import erf
    return np.vectorize(erf, otypes=[np.float64])(x)


def act64(v, act, slope):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_LRELU:
        return np.where(v >= 0, v, v * np.float64(np.float32(slope)))
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SWISH:
        return v / (1.0 + np.exp(-v))
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + _erf64(v / np.sqrt(2.0)))
    return v


def act32(v, act, slope):
    """The same functions evaluated by numpy in float32 (every step rounded to float32)."""
    v = v.astype(np.float32)
    one, s = np.float32(1.0), np.float32(slope)
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0))
    if act == ACT_LRELU:
        return np.where(v >= 0, v, v * s)
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SWISH:
        return v * (one / (one + np.exp(-v)))
    if act == ACT_GELU:
        # float32 erf: numpy has none; float64 erf rounded to float32 is the correctly rounded float32 erf, then float32 arithmetic
        e = _erf64((v * np.float32(0.70710678118654752440)).astype(np.float64)).astype(np.float32)
        return np.float32(0.5) * v * (one + e)
    return v


def act_deviation(pre32, act, slope) -> float:
    """Largest |float32 evaluation - float64 evaluation| of the activation on the float32 pre-activations `pre32`."""
    if act not in TRANSCENDENTAL or pre32.size == 0:
        return 0.0
    return float(np.max(np.abs(act32(pre32, act, slope).astype(np.float64) - act64(pre32.astype(np.float64), act, slope))))


# ---------------------------------------------------------------- convolution: data
def conv_data(c):
    """Seeded inputs of a case: in [B, T, Cin], w [Cout, KW, Cin] (tap-major), bias, res, out_old (float32)."""
    r = rng_of(c["name"])
    B, T, Cin, Cout, KW = c["B"], c["T"], c["Cin"], c["Cout"], c["KW"]
    d = dict(x=r.standard_normal((B, T, Cin), np.float32), w=(r.standard_normal((Cout, KW, Cin), np.float32) / np.float32(np.sqrt(KW * Cin))))
    if c["zts"]:   # polyphase upsampler: columns < split never use tap 2, columns >= split never tap 0
        d["w"][:c["zts"], 2, :] = 0
        d["w"][c["zts"]:, 0, :] = 0
    d["bias"] = r.standard_normal(Cout, np.float32) if c["bias"] else None
    d["res"] = r.standard_normal((B, T, Cout), np.float32) if c["res"] else None
    d["old"] = r.standard_normal((B, T, Cout), np.float32) if c["accumulate"] else None
    return d


def conv_gather(c, x):
    """f(in)[b, t - pad + j dil, c] as [B, T, KW, Cin] float32, zeros outside [0, T); f = max(x, x * in_slope) in float32."""
    B, T, Cin = x.shape
    s = np.float32(c["in_slope"])
    if c["in_slope"] != 1.0:
        x = np.maximum(x, x * s)
    a = np.zeros((B, T, c["KW"], Cin), np.float32)
    for j in range(c["KW"]):
        off = j * c["dil"] - c["pad"]
        lo, hi = max(0, -off), min(T, T - off)
        if hi > lo:
            a[:, lo:hi, j, :] = x[:, lo + off:hi + off, :]
    return a


def conv_pairs(c, d, x3, lo_round=bf16_round):
    """The operand pairs (A [B, T, KW, Cin], W [Cout, KW, Cin]) whose products the kernel sums, in the order it issues them."""
    a, w = conv_gather(c, d["x"]), d["w"]
    if x3 == 0:
        return [(a, w)]
    ah, al = split_bf16(a, lo_round)
    wh, wl = split_bf16(w, lo_round)
    return [(al, wh), (ah, wl), (ah, wh)] if x3 == 1 else [(ah, wh)]


def written_mask(c, bm=256):
    """[B, T] bool: rows the contract says are computed (t < act_rows[b]); and rows that are certainly left alone: t >= act_rows[b] rounded up
    to the row tile `bm` of the kernel that runs (kernels skip WHOLE tiles past act_rows; rows of the last tile past it may be written)."""
    B, T = c["B"], c["T"]
    t = np.arange(T)[None, :]
    if c["act_rows"] is None:
        return np.ones((B, T), bool), np.zeros((B, T), bool)
    ar = np.clip(np.asarray(c["act_rows"]), 0, T)[:, None]
    return t < ar, t >= (ar + bm - 1) // bm * bm


# ---------------------------------------------------------------- convolution: float64 reference and bars
def conv_reference(c, d, x3):
    """dict(ref, bar, S, pre32, dev, linear): the float64 result [B, T, Cout], the per-element bar, the sum of |terms|, ..."""
    pairs = conv_pairs(c, d, x3)
    B, T, Cout = c["B"], c["T"], c["Cout"]
    K = c["KW"] * c["Cin"]
    lin = np.zeros((B * T, Cout))
    S = np.zeros((B * T, Cout))
    for a, w in pairs:
        a2, w2 = a.reshape(B * T, K).astype(np.float64), w.reshape(Cout, K).astype(np.float64)
        lin += a2 @ w2.T
        S += np.abs(a2) @ np.abs(w2).T
    lin, S = lin.reshape(B, T, Cout), S.reshape(B, T, Cout)
    n = len(pairs) * K
    if d["bias"] is not None:
        lin = lin + d["bias"].astype(np.float64)
        S = S + np.abs(d["bias"]).astype(np.float64)
        n += 1
    act, slope = c["act"], c["act_slope"]
    e = gamma(n) * S                                     # bar of the pre-activation
    pre32 = lin.astype(np.float32)
    dev = act_deviation(pre32, act, slope)
    y = act64(lin, act, slope)
    if act == ACT_LRELU:
        e = gamma(n + 1) * S                             # one more multiplication
    elif act in TRANSCENDENTAL:
        e = LIPSCHITZ[act] * e + AGG_FACTOR * dev
        S = LIPSCHITZ[act] * S                           # |f(v)| <= L |v|: keeps err / S meaningful (not used by the aggregate bar)
    tail, St = 0, np.abs(y)
    if d["res"] is not None:
        y = y + d["res"].astype(np.float64)
        St = St + np.abs(d["res"])
        S = S + np.abs(d["res"])
        tail += 1
    if c["lens"] is not None:
        keep = (np.arange(T)[None, :] < np.asarray(c["lens"])[:, None])[:, :, None]
        y, e, S, St = y * keep, e * keep, S * keep, St * keep
    if d["old"] is not None:
        y = y + d["old"].astype(np.float64)
        St = St + np.abs(d["old"])
        S = S + np.abs(d["old"])
        tail += 1
    if c["out_div"] != 1.0:
        dv = np.float64(np.float32(c["out_div"]))
        y, e, S, St = y / dv, e / dv, S / dv, St / dv
        tail += 1
    e = e + gamma(tail + 1) * St if tail else e
    return dict(ref=y, bar=e, S=S, dev=dev, linear=act not in TRANSCENDENTAL, n=n + tail)


# ---------------------------------------------------------------- convolution: float32 evaluations (and their mutations)
def conv_eval32(c, d, x3, order="blocked", mut=None):
    """A float32 numpy evaluation of the operand model: one rounded product and one rounded addition per term (the bf16 products are exact).
    order 'blocked' (the yardstick): K in 32-channel chunks as the kernel walks it -- chunk-major, then tap, then channel, the product kinds
    of a term next to each other; 'sequential': tap-major, every channel of a tap in turn; 'matmul': chunk-major with one float32 matrix
    product (BLAS: wide partial sums, fused multiply-adds) per (chunk, tap, kind).  mut: a mutation (tests only), one of
    drop_tap, shift_tile, drop_tail_chunk, drop_split, trunc_lo, stale_col, mask_off_by_one, div_before."""
    lo_round = bf16_trunc if mut == "trunc_lo" else bf16_round
    pairs = conv_pairs(c, d, x3, lo_round)
    B, T, Cin, Cout, KW = c["B"], c["T"], c["Cin"], c["Cout"], c["KW"]
    if mut == "drop_split":
        assert x3 == 1
        pairs = pairs[1:]                                 # lo_a * hi_w never issued
    if mut == "shift_tile" and T > 64:                    # the rows of the tile that starts at row 64 read tap 0 one row late
        pairs = [(a.copy(), w) for a, w in pairs]
        for a, _ in pairs:
            a[:, 64:min(T, 128) - 1, 0, :] = a[:, 65:min(T, 128), 0, :]
    nchunk = (Cin + 31) // 32
    acc = np.zeros((B * T, Cout), np.float32)
    flat = [(a.reshape(B * T, KW, Cin), w) for a, w in pairs]

    def unit(j, c0, c1):   # the products of tap j, channels c0 .. c1 - 1
        for k in range(c0, c1):
            for a, w in flat:
                if order == "matmul":
                    continue
                np.add(acc, a[:, j, k:k + 1] * w[None, :, j, k], out=acc)
        if order == "matmul":
            for a, w in flat:
                np.add(acc, a[:, j, c0:c1] @ w[:, j, c0:c1].T, out=acc)

    if order == "sequential":
        assert mut is None
        for j in range(KW):
            unit(j, 0, Cin)
    else:
        for ch in range(nchunk):
            c0, c1 = ch * 32, min(Cin, ch * 32 + 32)
            if mut == "drop_tail_chunk" and ch == nchunk - 1:
                assert Cin % 32
                continue
            for j in range(KW):
                if mut == "drop_tap" and j == KW - 1 and ch == 0:
                    continue                              # one (tap, chunk) unit of the last tap skipped
                unit(j, c0, c1)
    v = acc.reshape(B, T, Cout)
    if d["bias"] is not None:
        v = v + d["bias"]
    v = act32(v, c["act"], c["act_slope"])
    if d["res"] is not None:
        v = v + d["res"]
    if c["lens"] is not None:
        lens = np.asarray(c["lens"]) + (1 if mut == "mask_off_by_one" else 0)
        v = v * (np.arange(T)[None, :] < lens[:, None])[:, :, None].astype(np.float32)
    dv = np.float32(c["out_div"])
    if mut == "div_before":
        assert d["old"] is not None and c["out_div"] != 1.0
        v = d["old"] + v / dv
    else:
        if d["old"] is not None:
            v = v + d["old"]
        if c["out_div"] != 1.0:
            v = v / dv
    v = v.astype(np.float32)
    if mut == "stale_col":
        assert Cout > 32
        v[:, :, 32] = np.float32(0.0)                     # the first column past a multiple of 32 never written (what a zeroed buffer holds)
    return v


def rel_rms(err, S):
    """Root mean square of err / S over the elements with S > 0."""
    m = S > 0
    if not np.any(m):
        return 0.0
    return float(np.sqrt(np.mean((err[m] / S[m]) ** 2)))


YARD_MAX_ROWS = 4224


def conv_yardstick(c, d, x3, ref):
    """RMS of err / S of the blocked float32 evaluation against float64 -- on the first utterances of the launch when it has more than
    YARD_MAX_ROWS rows (the statistic is a property of the operand model and the data's distribution, not of the launch size)."""
    Bs = c["B"] if c["B"] * c["T"] <= YARD_MAX_ROWS else max(1, YARD_MAX_ROWS // c["T"])
    cs = dict(c, B=Bs, lens=c["lens"][:Bs] if c["lens"] is not None else None, act_rows=c["act_rows"][:Bs] if c["act_rows"] is not None else None)
    ds = {k: (v[:Bs] if k in ("x", "res", "old") and v is not None else v) for k, v in d.items()}
    rows = written_mask(cs)[0]
    yerr = np.abs(conv_eval32(cs, ds, x3).astype(np.float64) - ref["ref"][:Bs])[rows]
    return rel_rms(yerr, ref["S"][:Bs][rows])


def check_conv(c, d, x3, got, ref=None, yard=None, rows=None):
    """Both bars on a result `got` [B, T, Cout] over the rows `rows` ([B, T] bool, default: every computed row).  yard: the yardstick
    statistic (conv_yardstick), computed when not given.  Returns dict(ok, elem_ratio (worst err / bar), agg_ratio (RMS statistic / 4 x the
    yardstick's, None when not applied), why)."""
    ref = ref or conv_reference(c, d, x3)
    if rows is None:
        rows = written_mask(c)[0]
    err = np.abs(got.astype(np.float64) - ref["ref"])[rows]
    bar, S = ref["bar"][rows], ref["S"][rows]
    finite = bool(np.all(np.isfinite(got[rows])))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    elem = float(ratio.max()) if ratio.size else 0.0
    agg = ys = None
    if ref["linear"] and err.size >= AGG_MIN_ELEMS:
        ys = conv_yardstick(c, d, x3, ref) if yard is None else yard
        gs = rel_rms(err, S)
        agg = gs / (AGG_FACTOR * ys) if ys > 0 else (0.0 if gs == 0 else np.inf)
    ys = ys if agg is not None else None
    ok = finite and elem <= 1.0 and (agg is None or agg <= 1.0)
    why = "" if ok else f"finite {finite}, worst err / bar {elem:.3g}, aggregate ratio {agg}"
    return dict(ok=ok, elem_ratio=elem, agg_ratio=agg, why=why, yard=ys if agg is not None else None)


def pack_x3(w):
    """[Cout, KW, Cin] float32 -> the split-precision image of ConvParams::w (packer.pack_x3's layout) as float32 words."""
    from e2e_tts_amd import packer
    Cout, KW, Cin = w.shape
    return packer.pack_x3(np.ascontiguousarray(w).reshape(Cout, KW * Cin), KW, Cin)


# ---------------------------------------------------------------- attention
def att_data(c):
    r = rng_of(c["name"])
    H = c["n_head"] * c["dk"]
    return dict(qkv=r.standard_normal((c["B"], c["N"], 3 * H), np.float32))


def _heads(c, qkv, dtype):
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    H = nh * dk
    q, k, v = (qkv[:, :, i * H:(i + 1) * H].reshape(B, N, nh, dk).transpose(0, 2, 1, 3).astype(dtype) for i in range(3))
    return q, k, v


def att_reference(c, d):
    """Masked softmax attention in float64: out [B, N, H], and W = sum_j p_j |v_j| per element.  Query rows >= lens[b] are 0."""
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    q, k, v = _heads(c, d["qkv"], np.float64)
    lens = np.full(B, N) if c["lens"] is None else np.asarray(c["lens"])
    s = q @ k.transpose(0, 1, 3, 2) / np.float64(np.float32(np.sqrt(np.float64(dk))))
    kmask = np.arange(N)[None, :] < lens[:, None]                      # [B, N]
    s = np.where(kmask[:, None, None, :], s, -np.inf)
    with np.errstate(invalid="ignore"):
        m = np.max(s, -1, keepdims=True)
        p = np.exp(s - np.where(np.isfinite(m), m, 0.0))
        p = p / np.where(p.sum(-1, keepdims=True) > 0, p.sum(-1, keepdims=True), 1.0)
    o, W = p @ v, p @ np.abs(v)
    qmask = kmask[:, None, :, None]
    o, W = np.where(qmask, o, 0.0), np.where(qmask, W, 0.0)
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(B, N, nh * dk)    # noqa: E731
    return back(o), back(W)


def att_eval32(c, d, x3=0, seg=None, drop_segment=False):
    """float32 numpy evaluation: scores, softmax and P V with every step in float32; x3: Q . K and P . V on split operands (the three
    products the kernel issues).  seg: keys per segment of an online-softmax evaluation (None: one pass); drop_segment (mutation): the
    last key segment never merged."""
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    q, k, v = _heads(c, d["qkv"], np.float32)
    lens = np.full(B, N) if c["lens"] is None else np.asarray(c["lens"])
    kmask = (np.arange(N)[None, :] < lens[:, None])[:, None, None, :]
    inv_t = np.float32(1.0) / np.float32(np.sqrt(np.float64(dk)))

    def mm(a, b):   # a @ b with float32 accumulation, on split operands in x3 mode
        if not x3:
            return a @ b
        ah, al = split_bf16(a)
        bh, bl = split_bf16(b)
        return (al @ bh + ah @ bl) + ah @ bh

    s = mm(q, np.ascontiguousarray(k.transpose(0, 1, 3, 2))) * inv_t
    s = np.where(kmask, s, np.float32(-np.inf))
    segs = [(0, N)] if not seg else [(a, min(N, a + seg)) for a in range(0, N, seg)]
    if drop_segment and len(segs) > 1:
        segs = segs[:-1]
    m_run = np.full((B, nh, N, 1), -np.inf, np.float32)
    l_run = np.zeros((B, nh, N, 1), np.float32)
    o = np.zeros((B, nh, N, dk), np.float32)
    with np.errstate(invalid="ignore"):
        for a, b in segs:
            sa = s[..., a:b]
            m_new = np.maximum(m_run, sa.max(-1, keepdims=True))
            m_use = np.where(np.isfinite(m_new), m_new, np.float32(0))
            corr = np.exp(np.where(np.isfinite(m_run), m_run, np.float32(-np.inf)) - m_use).astype(np.float32)
            p = np.exp(sa - m_use).astype(np.float32)
            l_run = l_run * corr + p.sum(-1, keepdims=True, dtype=np.float32)
            o = o * corr + mm(p, v[:, :, a:b, :])
            m_run = m_new
        o = o * (np.float32(1.0) / np.where(l_run > 0, l_run, np.float32(1.0)))
    qmask = (np.arange(N)[None, :] < lens[:, None])[:, None, :, None]
    o = np.where(qmask, o, np.float32(0))
    return o.transpose(0, 2, 1, 3).reshape(B, N, nh * dk).astype(np.float32)


def att_bar(c, d, x3, ref=None):
    """(ref, W, dev): the bar of an element is 4 x dev x W, dev = the largest |float32 evaluation - float64| / W of this case."""
    o, W = ref or att_reference(c, d)
    e = np.abs(att_eval32(c, d, x3, seg=32).astype(np.float64) - o)
    m = W > 0
    dev = float(np.max(e[m] / W[m])) if np.any(m) else 0.0
    return o, W, dev


def check_att(got, o, W, dev, rows=None):
    """rows: [B, N] bool of the rows to judge.  Returns (ok, worst err / bar)."""
    e = np.abs(got.astype(np.float64) - o)
    bar = AGG_FACTOR * dev * W
    if rows is not None:
        e, bar = e[rows], bar[rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, e / bar, np.where(e == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    return bool(np.all(np.isfinite(got))) and worst <= 1.0, worst


# ---------------------------------------------------------------- relative-position attention (kernels.h: launch_rel_attention)
def rel_data(c):
    r = rng_of(c["name"])
    H = c["n_head"] * c["dk"]
    return dict(qkv=r.standard_normal((c["B"], c["N"], 3 * H), np.float32), pos=r.standard_normal((c["n_head"], c["pos_rows"], c["dk"]), np.float32),
                u=(0.5 * r.standard_normal(H)).astype(np.float32), v=(0.5 * r.standard_normal(H)).astype(np.float32))


def rel_scores(c, d, dtype, x3=False, mut=None):
    """((q + u) . k + shift((q + v) . P)) / sqrt(H) as [B, heads, N, N], shift as kernels.h spells it out:
    (i, j <= i) -> (q_i + v) . P[N - 1 - i + j]; (i, i + 1) -> 0; (i, j > i + 1) -> (q_{i+1} + v) . P[j - i - 2]."""
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    q, k, _ = _heads(c, d["qkv"], np.float32)
    qu = (q + d["u"].reshape(1, nh, 1, dk)).astype(np.float32)         # formed in float32, as the kernel forms them
    qv = (q + d["v"].reshape(1, nh, 1, dk)).astype(np.float32)
    P = d["pos"]

    def mm(a, b):
        if not x3:
            return a.astype(dtype) @ b.astype(dtype)
        ah, al = split_bf16(a)
        bh, bl = split_bf16(b)
        ah, al, bh, bl = (t.astype(dtype) for t in (ah, al, bh, bl))
        return (al @ bh + ah @ bl) + ah @ bh

    content = mm(qu, np.ascontiguousarray(k.transpose(0, 1, 3, 2)))
    full = mm(qv, np.ascontiguousarray(P.transpose(0, 2, 1))[None])    # [B, nh, N, pos_rows]: (q_i + v) . P[r]
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    low = j <= i
    r_low = np.where(low, N - 1 - i + j, 0)
    if mut == "row":                                   # mutation (tests only): the lower triangle reads the table one row early
        r_low = np.maximum(r_low - 1, 0)
    r_up = np.where(j > i + 1, j - i - 2, 0)
    i_up = np.minimum(i + 1, N - 1) + 0 * j
    pos_s = np.where(low, full[:, :, i + 0 * j, r_low], np.where(j > i + 1, full[:, :, i_up, r_up], 0))
    if mut == "diag":                                  # mutation (tests only): entry (i, i + 1) taken from the table instead of 0
        pos_s = np.where(j == i + 1, full[:, :, i + 0 * j, np.zeros_like(r_up)], pos_s)
    H = nh * dk
    return ((content + pos_s) / dtype(np.float32(np.sqrt(np.float32(H))))).astype(dtype)


def rel_reference(c, d):
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    _, _, v = _heads(c, d["qkv"], np.float64)
    s = rel_scores(c, d, np.float64)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(B, N, nh * dk)    # noqa: E731
    return back(p @ v), back(p @ np.abs(v))


def rel_eval32(c, d, x3=False, mut=None):
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    _, _, v = _heads(c, d["qkv"], np.float32)
    s = rel_scores(c, d, np.float32, x3, mut)
    p = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32)
    if x3:
        ph, pl = split_bf16(p)
        vh, vl = split_bf16(v)
        o = (pl @ vh + ph @ vl) + ph @ vh
    else:
        o = p @ v
    o = o / p.sum(-1, keepdims=True, dtype=np.float32)
    return o.transpose(0, 2, 1, 3).reshape(B, N, nh * dk).astype(np.float32)


def rel_bar(c, d, x3):
    o, W = rel_reference(c, d)
    e = np.abs(rel_eval32(c, d, x3).astype(np.float64) - o)
    return o, W, float(np.max(e / W))


# ---------------------------------------------------------------- LayerNorm
def ln_data(c):
    r = rng_of(c["name"])
    x = (r.standard_normal((c["B"], c["N"], c["C"])) * 2 + 0.5).astype(np.float32)
    x[0, 0, :] = np.float32(1.25)              # rows of constant value: zero variance
    x[-1, -1, :] = np.float32(0.0)
    return dict(x=x, gamma=r.standard_normal(c["C"], np.float32), beta=r.standard_normal(c["C"], np.float32), eps=1e-5)


def ln_reference(c, d):
    """(ref, bar).  y = (x - mean) * rstd * gamma + beta, biased variance; rows t >= lens[b] are 0.  Bar: the mean and the variance are
    sums of C terms (gamma_{C+2} relative to mean|x| and to the variance + eps); propagated: |dy| <= |gamma| rstd (|d mean| + |x - mean|
    (d var / (2 (var + eps)) + 4 u)) + u (|y| + |beta|), doubled for the second-order terms."""
    x = d["x"].astype(np.float64)
    C = c["C"]
    eps = np.float64(np.float32(d["eps"]))
    mean = x.mean(-1, keepdims=True)
    xc = x - mean
    var = (xc ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    g, b = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    y = xc * rstd * g + b
    gC = gamma(C + 2)
    dmean = gC * np.abs(x).mean(-1, keepdims=True)
    dxc = dmean + U * (np.abs(x) + np.abs(mean))
    dvar = gC * var + 2 * (np.abs(xc) * dxc).mean(-1, keepdims=True) + (dxc ** 2).mean(-1, keepdims=True)
    drstd = rstd * (dvar / (2 * (var + eps)) + 4 * U)
    bar = 2 * (np.abs(g) * (rstd * dxc + np.abs(xc) * drstd + 2 * U * np.abs(xc) * rstd) + U * (np.abs(y) + np.abs(b)))
    if c["lens"] is not None:
        keep = (np.arange(c["N"])[None, :] < np.asarray(c["lens"])[:, None])[:, :, None]
        y, bar = y * keep, bar * keep
    return y, bar


def ln_eval32(c, d):
    x = d["x"]
    C = np.float32(c["C"])
    mean = (x.sum(-1, keepdims=True, dtype=np.float32) / C).astype(np.float32)
    xc = x - mean
    var = ((xc * xc).sum(-1, keepdims=True, dtype=np.float32) / C).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = np.float32(1.0) / np.sqrt(var + np.float32(d["eps"]))
        y = xc * rstd * d["gamma"] + d["beta"]
    if c["lens"] is not None:
        y = y * (np.arange(c["N"])[None, :] < np.asarray(c["lens"])[:, None])[:, :, None]
    return y.astype(np.float32)


# ---------------------------------------------------------------- small kernels
def post_data(c, small=False):
    """Inputs with |wav| well inside (-1, 1).  small: weights and bias scaled down until the worst-case bar of a sample, gamma_n S, is so far
    below one PCM step that at most ~0.05 % of the samples lie within it of a rounding boundary (the share of such samples is about
    2 x 32768 x bar): the only inputs for which the PCM comparison's exclusion rule stays under the project's 0.1 % share."""
    r = rng_of(c["name"])
    B, N, C, KW = c["B"], c["N"], c["C"], c["KW"]
    xs = [r.standard_normal((B, N, C), np.float32) for _ in range(1 + c["n_add"])]
    w, bias = r.standard_normal((KW, C)) * 0.6 / np.sqrt(KW * C), 0.05
    if small:
        s_typ = 0.6 * np.sqrt(KW * C) + 0.05                      # about the largest S at unit scale
        f = 2.5e-4 / (2 * 32768 * float(gamma(KW * C + 1)) * s_typ)
        w, bias = w * f, bias * f
    return dict(xs=xs, w=w.astype(np.float32), bias=np.array([bias], np.float32))


def post_reference(c, d):
    """(wav float64 [B, N], bar): x = (((x + a0) + a1) + a2) / x_div formed in float32 (the kernel's own operand), lrelu 0.01 in float32,
    conv with zero padding (KW - 1) / 2, + bias, tanh."""
    x = d["xs"][0]
    for a in d["xs"][1:]:
        x = x + a
    if c["n_add"] and c["x_div"] != 1.0:
        x = x / np.float32(c["x_div"])
    x = np.where(x >= 0, x, x * np.float32(0.01)).astype(np.float32)
    B, N, C, KW = c["B"], c["N"], c["C"], c["KW"]
    pad = (KW - 1) // 2
    xp = np.zeros((B, N + KW - 1, C), np.float64)
    xp[:, pad:pad + N] = x
    w = d["w"].astype(np.float64)
    lin, S = np.zeros((B, N)), np.zeros((B, N))
    for j in range(KW):
        lin += xp[:, j:j + N] @ w[j]
        S += np.abs(xp[:, j:j + N]) @ np.abs(w[j])
    lin, S = lin + np.float64(d["bias"][0]), S + abs(float(d["bias"][0]))
    pre32 = lin.astype(np.float32)
    dev = float(np.max(np.abs(np.tanh(pre32).astype(np.float64) - np.tanh(pre32.astype(np.float64)))))
    return np.tanh(lin), gamma(KW * C + 1) * S + AGG_FACTOR * dev, dev


def pcm_of(wav32):
    """(int16)(int32)(wav * 32768) of a float32 waveform: the product in float32, truncation toward zero, wrap to 16 bits."""
    v = (wav32.astype(np.float32) * np.float32(32768.0)).astype(np.float32)
    return np.trunc(v).astype(np.int64).astype(np.int32).astype(np.int16)


def pcm_boundary(wav64, bar):
    """Samples whose reference value lies within `bar` of a rounding boundary of the conversion (an integer of wav * 32768): there the
    kernel's PCM may differ by more than what the 1-LSB comparison allows for."""
    v = wav64 * 32768.0
    return np.abs(v - np.round(v)) <= bar * 32768.0


def dw_data(c, glu=False):
    r = rng_of(c["name"] + ("_glu" if glu else ""))
    B, N, C, k = c["B"], c["N"], c["C"], c["k"]
    return dict(x=r.standard_normal((B, N, 2 * C if glu else C), np.float32), w=(r.standard_normal((k, C)) / np.sqrt(k)).astype(np.float32),
                bias=r.standard_normal(C, np.float32))


def glu32(x):
    C = x.shape[-1] // 2
    return (x[..., :C] * (np.float32(1) / (np.float32(1) + np.exp(-x[..., C:])))).astype(np.float32)


def glu_reference(x):
    """(ref, bar): a * sigmoid(g); bar = 4 x the float32 evaluation's largest deviation relative to |a| ... applied as dev * |a| + u |ref|."""
    C = x.shape[-1] // 2
    a, g = x[..., :C].astype(np.float64), x[..., C:].astype(np.float64)
    ref = a / (1.0 + np.exp(-g))
    dev = float(np.max(np.abs(glu32(x).astype(np.float64) - ref) / np.maximum(np.abs(a), 1e-300)))
    return ref, AGG_FACTOR * dev * np.abs(a) + U * np.abs(ref), dev


def dw_reference(c, x, w, bias):
    """Depthwise conv over [0, N) with zero padding (k - 1) / 2, + bias, swish, from a float32 input x [B, N, C]: (ref, bar, dev)."""
    B, N, C = x.shape
    k = c["k"]
    half = (k - 1) // 2
    xp = np.zeros((B, N + k - 1, C))
    xp[:, half:half + N] = x
    lin, S = np.zeros((B, N, C)), np.zeros((B, N, C))
    for j in range(k):
        lin += xp[:, j:j + N] * w[j].astype(np.float64)
        S += np.abs(xp[:, j:j + N]) * np.abs(w[j]).astype(np.float64)
    lin, S = lin + bias.astype(np.float64), S + np.abs(bias).astype(np.float64)
    pre32 = lin.astype(np.float32)
    dev = act_deviation(pre32, ACT_SWISH, 0.0)
    return act64(lin, ACT_SWISH, 0.0), LIPSCHITZ[ACT_SWISH] * gamma(k + 1) * S + AGG_FACTOR * dev, dev


# ---------------------------------------------------------------- 16-bit activations (precisions "bf16_act" / "fp16_act")
# Written from BConvParams / PairParams (csrc/kernels.h) and the rounding tables of include/e2etts.h.  A 16-bit tensor is handled here as a
# float32 array that holds 16-bit values (exact both ways); bits16 / from_bits16 move between that and the uint16 patterns the kernels see.
#
# Exact tier.  Activations, weights and bias are drawn from small dyadic grids, so every product is a multiple of one `unit` and every
# partial sum of an output element, in ANY order, is a multiple of `unit` below 2^24 units: exactly representable in float32.  An
# fp32-accumulating kernel must then deliver the exact sum whatever its order of terms, and the elementwise tail (one float32 operation on
# 16-bit values and one nearest-even rounding per step) is fully determined: the kernel's output equals a16_exact() bit for bit.  The
# precondition max S / unit < 2^24 (S = sum of |terms| of an element, bias included; unit = lowest set bit over the staged activations x
# lowest set bit over the weights, and it divides the bias) is what act16_exactness() returns; tests/test_kernel_ref_host.py asserts it for
# every case.  Residual and running sum enter after the accumulation and are arbitrary 16-bit data.
#
# General tier.  Gaussian data (non-dyadic conversions, rounding of the staged operands) under two rules: the interval rule -- every step of
# the tail is monotone non-decreasing, so with ref the float64 sum over the staged 16-bit operands and bar = gamma_n S each output lies in
# [chain(ref - bar), chain(ref + bar)], endpoints rounded outward to float32, no element excluded --, and the aggregate rule -- the share of
# elements whose bits differ from chain(fl32(ref)) is at most AGG_FACTOR x the same share of conv_eval32 (blocked order) plus one element.
# The aggregate rule needs flips to count, so its data carry a per-channel mean that the bias cancels (a16_data); plain zero-mean Gaussian
# data, the distribution the engine sees and the one with the tightest intervals, goes under the interval rule at the case's own size.
A16_BF16, A16_FP16 = 1, 2
A16_NAME = {A16_BF16: "bf16_act", A16_FP16: "fp16_act"}
A16_EXACT_LIMIT = 2.0 ** 24
A16_GENERAL_MEAN = 6.0


def act16_round(x, kind, how="rne"):
    """float32 -> the nearest value of the element type (1: bf16, 2: IEEE binary16), ties to even, overflow to infinity, subnormals kept;
    returned as float32.  how (mutations, tests only): 'rtz' rounds toward zero, 'rha' sends ties away from zero, 'sat' saturates fp16 overflow at 65504, 'ftz' flushes
    fp16 subnormal results to zero."""
    x = np.ascontiguousarray(x, np.float32)
    if how == "rha":             # mutation: ties away from zero instead of to even
        if kind == A16_BF16:
            u = x.view(np.uint32)
            return (((u + np.uint32(0x8000)) >> np.uint32(16)) << np.uint32(16)).view(np.float32)
        with np.errstate(over="ignore"):
            r = x.astype(np.float16)
            dn = np.where(np.abs(r.astype(np.float32)) > np.abs(x), np.nextafter(r, np.float16(0)), r)
            up = np.nextafter(dn, np.copysign(np.float16(np.inf), x).astype(np.float16))
            tie = np.isfinite(up) & (np.abs(x.astype(np.float64) - dn.astype(np.float64)) == np.abs(up.astype(np.float64) - x.astype(np.float64)))
        return np.where(tie, up, r).astype(np.float32)
    if how == "rtz":
        if kind == A16_BF16:
            return bf16_trunc(x)
        with np.errstate(over="ignore"):
            r = x.astype(np.float16).astype(np.float32)
            back = np.nextafter(x.astype(np.float16), np.float16(0)).astype(np.float32)
        return np.where(np.abs(r) > np.abs(x), back, r).astype(np.float32)
    if kind == A16_BF16:
        return bf16_round(x)
    with np.errstate(over="ignore"):
        r = x.astype(np.float16).astype(np.float32)
    if how == "sat":
        r = np.where(np.isinf(r) & np.isfinite(x), np.sign(x) * np.float32(65504.0), r).astype(np.float32)
    if how == "ftz":
        r = np.where(np.abs(r) < np.float32(2.0 ** -14), np.copysign(np.float32(0), r), r).astype(np.float32)
    return r


def bits16(x, kind):
    """float32 holding 16-bit values -> their uint16 patterns (rounds to nearest-even when it does not)."""
    if kind == A16_FP16:
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(np.asarray(x, np.float32).astype(np.float16)).view(np.uint16)
    return (np.ascontiguousarray(bf16_round(x)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def from_bits16(u, kind):
    u = np.ascontiguousarray(u, np.uint16)
    return u.view(np.float16).astype(np.float32) if kind == A16_FP16 else (u.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _lrelu32(v, slope):
    """max(v, v * slope) in float32: BConvParams::act_slope / in_slope (slope in [0, 1]; 1 = identity)."""
    return np.maximum(v, v * np.float32(slope)).astype(np.float32)


def act16_stage(c, kind, x, adds=(), how="rne", drop_join=None):
    """The operand a convolution stages from its input, float32 holding 16-bit values; the three forms of BConvParams:
    fp32 input: round(lrelu(x)); 16-bit input: round(lrelu(x)), a slope of 1 copies; 16-bit join (in_add): x = r(r(r(in + a0) + a1) + a2),
    then r(x / in_div), then r(lrelu(x)).  drop_join (mutation): index of a join rounding to leave out."""
    r = lambda v: act16_round(v, kind, how)   # noqa: E731
    x = np.asarray(x, np.float32)
    slope = c["in_slope"]
    if not c["in16"]:
        assert not adds
        return r(_lrelu32(x, slope) if slope != 1.0 else x)
    if not adds:
        return x if slope == 1.0 else r(_lrelu32(x, slope))
    v = x
    for i, a in enumerate(adds):
        v = (v + np.asarray(a, np.float32)).astype(np.float32)
        if drop_join != i:
            v = r(v)
    if c["in_div"] != 1.0:
        v = r((v / np.float32(c["in_div"])).astype(np.float32))
    return r(_lrelu32(v, slope))


def act16_chain(pre32, c, res16, old16, kind, how="rne", mut=None):
    """The epilogue of conv_bf16_kernel with 16-bit activations on pre32 = fl32(accumulator + bias): round; activation, round; + residual,
    round; + running sum, round; / out_div, round -- each step present only when the launch asks for it.  mut (tests only): 'drop_bias_round',
    'res_before_act', 'div_before'."""
    r = lambda v: act16_round(v, kind, how)   # noqa: E731
    v = np.asarray(pre32, np.float32)
    if mut != "drop_bias_round":
        v = r(v)
    if mut == "res_before_act" and res16 is not None:
        v = r((v + res16).astype(np.float32))
    if c["act_slope"] != 1.0:
        v = r(_lrelu32(v, c["act_slope"]))
    if res16 is not None and mut != "res_before_act":
        v = r((v + res16).astype(np.float32))
    dv = np.float32(c["out_div"])
    if mut == "div_before":
        assert old16 is not None and c["out_div"] != 1.0
        return r((old16 + r((v / dv).astype(np.float32))).astype(np.float32))
    if old16 is not None:
        v = r((v + old16).astype(np.float32))
        if c["out_div"] != 1.0:
            v = r((v / dv).astype(np.float32))
    return v


def _grid(r, shape, kmax, exp, neg=None, kmin=0):
    k = r.integers(-kmax, kmax + 1, shape)
    if kmin:                     # |k| in [kmin, kmax]
        k = r.integers(kmin, kmax + 1, shape) * r.choice(np.array([-1, 1]), shape)
    if neg is not None:          # negatives restricted to a few coarse values (a non-dyadic staging slope)
        k = np.where(k < 0, np.asarray(neg)[r.integers(0, len(neg), shape)], k)
    return (k * 2.0 ** exp).astype(np.float32)


def a16_grids(c, kind):
    """(x, w, addend, fine bits of an fp32 input) grids of a case as (kmax, exponent).  Default: x in {-48..48} 2^-4, w in {-16..16} 2^-6,
    bias on the x grid; for fp16 both finer by 2^-2 (unless the case says fine16 = False).  Addends of a join lie on a finer grid than x so
    that the join's roundings change their sums; an fp32 input carries `fb` more bits than the element type keeps, for the same reason."""
    sh = -2 if (kind == A16_FP16 and c["fine16"]) else 0
    xg = (c["xg"][0], c["xg"][1] + sh)
    wg = (c["wg"][0], c["wg"][1] + sh)
    ag = c["ag"][kind] if isinstance(c["ag"], dict) else c["ag"] if c["ag"] is not None else ((48, xg[1] - 3) if kind == A16_BF16 else (48, xg[1] - 7))
    fb = c["fb"] if c["fb"] is not None else (3 if kind == A16_BF16 else 6)
    return xg, wg, ag, fb


def a16_data(c, kind, tier="exact"):
    """Seeded inputs of a 16-bit-activation case: x [B, T, Cin] (float32; 16-bit values when the case's input is 16-bit), adds, w
    [Cout, KW, Cin] float32, bias, res, old (16-bit values).  tier 'exact': grid data; 'general': Gaussian about a per-channel mean;
    'zero_mean': plain Gaussian."""
    r = rng_of(f"{c['name']}/{kind}/{tier}")
    B, T, Cin, Cout, KW = c["B"], c["T"], c["Cin"], c["Cout"], c["KW"]
    rnd = lambda v: act16_round(v, kind)   # noqa: E731
    if tier == "exact":
        xg, wg, ag, fb = a16_grids(c, kind)
        if c["in16"]:
            x = _grid(r, (B, T, Cin), xg[0], xg[1], c["neg"], c["kmin"])
            assert np.array_equal(x, rnd(x)), "the x grid is not representable in the element type"
        else:
            x = _grid(r, (B, T, Cin), xg[0] << fb, xg[1] - fb)
        adds = [_grid(r, (B, T, Cin), ag[0], ag[1]) for _ in range(c["n_add"])]
        w = _grid(r, (Cout, KW, Cin), wg[0], wg[1])
        assert np.array_equal(w, rnd(w)) and all(np.array_equal(a, rnd(a)) for a in adds)
        bias = _grid(r, (Cout,), xg[0], xg[1]) if c["bias"] else None
        rs = np.float32(c["xg"][0] * 2.0 ** xg[1] / 3)          # residual / running sum: arbitrary 16-bit data of the x grid's magnitude
    else:
        # Gaussian about a mean of A16_GENERAL_MEAN standard deviations whose sign goes with the channel, in x and in w alike: the products
        # of a channel then share a sign, the partial sums grow an order of magnitude past the result, and the bias (below) takes the
        # columns' mean sum away again.  Zero-mean data leaves a float32 order difference so little room to move a 16-bit result (a share
        # of 4e-6 for bf16) that the aggregate rule would compare counts of 0, 1 and 2.
        # tier 'zero_mean': plain Gaussian data, the ordinary distribution; judged by the interval rule alone.
        mean = 0.0 if tier == "zero_mean" else A16_GENERAL_MEAN
        sgn = r.choice(np.array([-1.0, 1.0], np.float32), Cin)
        x = (r.standard_normal((B, T, Cin), np.float32) + np.float32(mean) * sgn).astype(np.float32)
        x = rnd(x) if c["in16"] else x
        adds = [rnd(r.standard_normal((B, T, Cin), np.float32)) for _ in range(c["n_add"])]
        w = ((r.standard_normal((Cout, KW, Cin), np.float32) + np.float32(mean) * sgn) / np.float32(max(mean, 1.0) * np.sqrt(KW * Cin)))
        bias = r.standard_normal(Cout, np.float32) if c["bias"] else None
        rs = np.float32(1.0)
    if c["zts"]:
        w[:c["zts"], 2, :] = 0
        w[c["zts"]:, 0, :] = 0
    if tier != "exact" and bias is not None:
        cc = dict(c, B=min(B, 4))
        lin = a16_sum64(cc, kind, dict(x=x[:4], adds=[a[:4] for a in adds], w=w, bias=None))[0]
        bias = (bias - lin.mean((0, 1))).astype(np.float32)
    res = rnd(rs * r.standard_normal((B, T, Cout), np.float32)) if c["res"] else None
    old = rnd(rs * r.standard_normal((B, T, Cout), np.float32)) if c["accumulate"] else None
    return dict(x=x, adds=adds, w=w, bias=bias, res=res, old=old)


def _a16_operands(c, kind, d, how="rne", drop_join=None):
    """(A [B T, K] float32, W [Cout, K] float32): the staged 16-bit operands, gathered tap-major."""
    st = act16_stage(c, kind, d["x"], d["adds"], how, drop_join)
    a = conv_gather(dict(c, in_slope=1.0), st)
    return a.reshape(c["B"] * c["T"], c["KW"] * c["Cin"]), act16_round(d["w"], kind).reshape(c["Cout"], c["KW"] * c["Cin"])


def _lsb(v):
    """The lowest set bit over the nonzero elements of a float32 array (inf when there is none)."""
    v = np.abs(np.asarray(v, np.float64).ravel())
    v = v[v > 0]
    if v.size == 0:
        return np.inf
    m, e = np.frexp(v)
    q = np.round(m * 2.0 ** 53).astype(np.int64)
    return float(np.min((q & -q).astype(np.float64) * 2.0 ** (e - 53)))


def act16_exactness(c, kind, d=None):
    """max over the output elements of S / unit for the exact-tier data of a case (A16_EXACT_LIMIT = 2^24 is the precondition of the
    tier); inf when the bias is no multiple of the unit.  Returns (ratio, unit)."""
    d = d or a16_data(c, kind)
    a, w = _a16_operands(c, kind, d)
    unit = _lsb(a) * _lsb(w)
    S = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    if d["bias"] is not None:
        q = d["bias"].astype(np.float64) / unit
        if not np.array_equal(q, np.round(q)):
            return np.inf, unit
        S = S + np.abs(d["bias"]).astype(np.float64)
    return float(S.max() / unit), unit


def a16_sum64(c, kind, d, how="rne", drop_join=None):
    """(ref, S, n): the float64 sum over the staged 16-bit operands plus the bias [B, T, Cout], the sum of |terms|, the number of terms."""
    a, w = _a16_operands(c, kind, d, how, drop_join)
    a, w = a.astype(np.float64), w.astype(np.float64)
    ref, S = a @ w.T, np.abs(a) @ np.abs(w).T
    n = c["KW"] * c["Cin"]
    if d["bias"] is not None:
        ref, S, n = ref + d["bias"].astype(np.float64), S + np.abs(d["bias"]).astype(np.float64), n + 1
    shp = (c["B"], c["T"], c["Cout"])
    return ref.reshape(shp), S.reshape(shp), n


def a16_exact(c, kind, d):
    """The exact tier's expected output (float32 holding 16-bit values): the exact sum, which under the tier's precondition is a float32,
    through the epilogue."""
    ref, _, _ = a16_sum64(c, kind, d)
    pre32 = ref.astype(np.float32)
    assert np.array_equal(pre32.astype(np.float64), ref), "the exact sum is no float32: the exactness condition does not hold"
    return act16_chain(pre32, c, d["res"], d["old"], kind)


def a16_eval32(c, kind, d, order="blocked", mut=None):
    """A float32 evaluation of the launch (conv_eval32's orders on the staged operands), through the epilogue.  mut (tests only):
    drop_bias_round, rtz, rha, res_before_act, div_before, drop_join, drop_tap_last_row, tail_not_zeroed, sat, ftz."""
    how = mut if mut in ("rtz", "rha", "sat", "ftz") else "rne"
    st = act16_stage(c, kind, d["x"], d["adds"], how, 0 if mut == "drop_join" else None)
    w16 = act16_round(d["w"], kind)
    cc = dict(c, in_slope=1.0, act=ACT_NONE, lens=None)
    dd = dict(x=st, w=w16, bias=None, res=None, old=None)
    if mut == "drop_tap_last_row":       # the slab's last row is never seen by the last tap: one output row loses one tap
        t = c["T"] - 1 + c["pad"] - (c["KW"] - 1) * c["dil"]
        assert 0 <= t < c["T"]
        acc = conv_eval32(dict(cc, accumulate=False, out_div=1.0), dd, 0, order)
        a_last = st[:, c["T"] - 1, :]                                     # [B, Cin]
        acc[:, t, :] = (acc[:, t, :] - a_last @ w16[:, c["KW"] - 1, :].T).astype(np.float32)
    else:
        acc = conv_eval32(dict(cc, accumulate=False, out_div=1.0), dd, 0, order)
    if mut == "tail_not_zeroed":         # the channels past Cin of the last 32-channel chunk hold the slab's clamped read instead of zeros
        assert c["Cin"] % 32
        ph = conv_gather(cc, st)[:, :, :, -8:].reshape(c["B"], c["T"], -1) @ w16[:, :, -8:].reshape(c["Cout"], -1).T
        acc = (acc + ph).astype(np.float32)
    pre32 = (acc + d["bias"]).astype(np.float32) if d["bias"] is not None else acc
    cm = mut if mut in ("drop_bias_round", "res_before_act", "div_before") else None
    return act16_chain(pre32, c, d["res"], d["old"], kind, how, cm)


def _outward32(v, up):
    f = v.astype(np.float32)
    with np.errstate(over="ignore"):
        if up:
            return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
        return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def a16_general_reference(c, kind, d):
    """dict(lo, hi, mid, one_value): the interval rule's endpoints [chain(ref - bar), chain(ref + bar)] (outward-rounded float32 through the
    epilogue), mid = chain(fl32(ref)), and the share of elements whose interval holds one value."""
    ref, S, n = a16_sum64(c, kind, d)
    bar = gamma(n) * S
    lo = act16_chain(_outward32(ref - bar, False), c, d["res"], d["old"], kind)
    hi = act16_chain(_outward32(ref + bar, True), c, d["res"], d["old"], kind)
    mid = act16_chain(ref.astype(np.float32), c, d["res"], d["old"], kind)
    return dict(lo=lo, hi=hi, mid=mid, one_value=float(np.mean(lo == hi)))


def flip_share(got, mid, kind):
    return float(np.mean(bits16(got, kind) != bits16(mid, kind)))


A16_GENERAL_ELEMS = (2 ** 18, 2 ** 17)     # K < 1024, K >= 1024


def a16_general_case(c):
    """The launch the general tier judges: the case with as many utterances as give the aggregate rule a count to compare -- a share of
    flips of 1e-4 (the float32 yardstick's at K = 24 with bf16 elements: u sqrt(K) against an ulp of 2^-8) is 0, 1 or 2 elements of a
    launch of 8192 by chance alone, whatever computed it; of 2^18 elements it is some twenty.  Same T, channels, kernel and options."""
    want = A16_GENERAL_ELEMS[0 if c["KW"] * c["Cin"] < 1024 else 1]
    per = c["T"] * c["Cout"]
    return dict(c, B=max(c["B"], -(-want // per)), rows_hint=c["rows_hint"] or c["B"] * c["T"])    # rows_hint: the tile shape the case names


def check_a16_interval(c, kind, d, got):
    """The interval rule alone (launches of zero-mean Gaussian data, at the case's own size): (elements outside, one-value share)."""
    ref = a16_general_reference(c, kind, d)
    with np.errstate(invalid="ignore"):
        inside = (got >= ref["lo"]) & (got <= ref["hi"])
    return int(np.sum(~inside)), ref["one_value"]


def check_a16_general(c, kind, d, got, ref=None, yard=None):
    """Both rules of the general tier on `got` (float32 holding 16-bit values).  yard: the flip share of conv_eval32's blocked order
    (computed when not given).  The aggregate rule applies to launches of at least AGG_MIN_ELEMS elements."""
    ref = ref or a16_general_reference(c, kind, d)
    with np.errstate(invalid="ignore"):
        inside = (got >= ref["lo"]) & (got <= ref["hi"])
    share = flip_share(got, ref["mid"], kind)
    agg_ok, ys = True, None
    if got.size >= AGG_MIN_ELEMS:
        ys = flip_share(a16_eval32(c, kind, d), ref["mid"], kind) if yard is None else yard
        agg_ok = share <= AGG_FACTOR * ys + 1.0 / got.size
    ok = bool(np.all(inside)) and agg_ok
    why = "" if ok else f"{int(np.sum(~inside))} elements outside their interval; flip share {share:.4g} against the yardstick's {ys}"
    return dict(ok=ok, outside=int(np.sum(~inside)), share=share, yard=ys, one_value=ref["one_value"], why=why)


def a16_image_reference(w, kind, tap_split=0):
    """The weight image of launch_bf16_image / launch_f16_image as uint16 [Cout / 32][chunk][tap slot][k-step 0..1][lane 0..63][8]: lane l of
    tile t holds output channel 32 t + l % 32, input channels 32 chunk + 16 k-step + 8 (l / 32) + 0..7, zeros past Cin; with tap_split
    (KW == 3) tap slot s of tile t is tap s + (32 t >= tap_split)."""
    Cout, KW, Cin = w.shape
    nch, KWe = (Cin + 31) // 32, (2 if tap_split else KW)
    wp = np.zeros((Cout, KW, nch * 32), np.float32)
    wp[:, :, :Cin] = w
    img = np.zeros((Cout // 32, nch, KWe, 2, 64, 8), np.uint16)
    b = bits16(wp, kind).reshape(Cout // 32, 32, KW, nch, 2, 2, 8)        # [tile, n, tap, chunk, k-step, half, 8]
    for t in range(Cout // 32):
        j0 = 1 if (tap_split and 32 * t >= tap_split) else 0
        for s in range(KWe):
            # -> [chunk, k-step, half, n, 8] -> lanes = half * 32 + n
            img[t, :, s] = b[t, :, s + j0].transpose(1, 2, 3, 0, 4).reshape(nch, 2, 64, 8)
    return img


# conv_post with 16-bit activations (launch_conv_post_bf16): x = r(lrelu_0.01(x)); y = r(conv + b); wav = r(tanh(y))
def post16_data(c, kind):
    r = rng_of(f"{c['name']}/post16/{kind}")
    B, N, C, KW = c["B"], c["N"], c["C"], c["KW"]
    rnd = lambda v: act16_round(v, kind)   # noqa: E731
    return dict(x=rnd(r.standard_normal((B, N, C), np.float32)), w=rnd((r.standard_normal((KW, C)) * 0.6 / np.sqrt(KW * C)).astype(np.float32)),
                bias=rnd(np.array([0.05], np.float32)))


def post16_reference(c, kind, d):
    """(lo, hi, dev): the interval of wav.  The pre-tanh sum is bracketed by gamma_n S, rounded; tanh is monotone, so wav lies in
    [r(tanh(r(ref - bar)) - a), r(tanh(r(ref + bar)) + a)], a = AGG_FACTOR x the float32 tanh's largest deviation from float64 on this
    case (post_reference's allowance for the device's tanhf)."""
    rnd = lambda v: act16_round(v, kind)   # noqa: E731
    x = d["x"]
    x = rnd(np.where(x >= 0, x, x * np.float32(0.01)).astype(np.float32))
    B, N, C, KW = c["B"], c["N"], c["C"], c["KW"]
    pad = (KW - 1) // 2
    xp = np.zeros((B, N + KW - 1, C), np.float64)
    xp[:, pad:pad + N] = x
    w = d["w"].astype(np.float64)
    lin, S = np.zeros((B, N)), np.zeros((B, N))
    for j in range(KW):
        lin += xp[:, j:j + N] @ w[j]
        S += np.abs(xp[:, j:j + N]) @ np.abs(w[j])
    lin, S = lin + np.float64(d["bias"][0]), S + abs(float(d["bias"][0]))
    bar = gamma(KW * C + 1) * S
    ylo, yhi = rnd(_outward32(lin - bar, False)), rnd(_outward32(lin + bar, True))
    dev = float(max(np.max(np.abs(np.tanh(y).astype(np.float64) - np.tanh(y.astype(np.float64)))) for y in (ylo, yhi)))
    a = AGG_FACTOR * dev
    lo = rnd(_outward32(np.tanh(ylo.astype(np.float64)) - a, False))
    hi = rnd(_outward32(np.tanh(yhi.astype(np.float64)) + a, True))
    return lo, hi, dev
