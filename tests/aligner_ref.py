"""numpy restatement of the reference's forced alignment, for the host tests and for geometries no fixture holds:

  * ``forward``: AlignmentEncoder.forward (U/layers.py:332-369) in float32 or float64 -- the speaker terms added to every position, the
    padded positions included, "same" zero-padded convolutions over the whole padded tensor, the squared distance in the direct form, the
    log-softmax over ALL key columns before the mask, the masked softmax;
  * ``mas_loops`` / ``b_mas``: the monotonic alignment search (what U/function.py:96-137 computes) as plain loops over cells with an explicit
    array of back-pointer bits; ``mas_rows`` is the same recurrence with each frame's columns computed at once (the same additions and
    comparisons, so the same path), for maps too large for the loops;
  * ``beta_binomial_prior`` / ``pad_prior``: the attention prior of the reference's data preparation (what src/tools/utils.py:129-139 and
    dataloader.py:274-281 compute).
Each is written in this project's own terms; that it equals the reference is what the fixtures prove (the reference's own functions made them).

U/ = e2e_tts/models/acoustic/unsupervised_fastspeech2/.  Weights are passed under the submodule's own state-dict names
("key_proj.0.conv.weight", ..., "query_spk_proj.linear.weight")."""
from __future__ import annotations

import numpy as np

PREFIX = "variance_adaptor.aligner."


def submodule_state(state, prefix=PREFIX):
    return {k[len(prefix):]: np.asarray(v) for k, v in state.items() if k.startswith(prefix)}


def conv1d_same(x, w, b):
    """x [B, Cin, N], w [Cout, Cin, K] (K odd), b [Cout] -> [B, Cout, N], zero padding (K - 1) / 2 per side (ConvNorm's default)."""
    K = w.shape[2]
    pad = (K - 1) // 2
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad)))
    N = x.shape[2]
    out = np.zeros((x.shape[0], w.shape[0], N), x.dtype)
    for j in range(K):
        out += np.einsum("oc,bcn->bon", w[:, :, j], xp[:, :, j:j + N])
    return out + b[None, :, None]


def log_softmax(a):
    m = a.max(-1, keepdims=True)
    return (a - m) - np.log(np.exp(a - m).sum(-1, keepdims=True))


def forward(P, queries, keys, temperature, txt_lens=None, prior=None, speaker=None, dtype=np.float32):
    """queries [B, n_mel, T], keys [B, n_text, L] (the reference's layouts) -> (attn, attn_logprob), both [B, T, L] in `dtype`."""
    W = {k: np.asarray(v).astype(dtype) for k, v in P.items()}
    q, k = np.asarray(queries).astype(dtype), np.asarray(keys).astype(dtype)
    if speaker is not None:
        s = np.asarray(speaker).astype(dtype)
        k = k + (s @ W["key_spk_proj.linear.weight"].T)[:, :, None]
        q = q + (s @ W["query_spk_proj.linear.weight"].T)[:, :, None]
    relu = lambda v: np.maximum(v, 0)  # noqa: E731
    ke = conv1d_same(relu(conv1d_same(k, W["key_proj.0.conv.weight"], W["key_proj.0.conv.bias"])), W["key_proj.2.conv.weight"], W["key_proj.2.conv.bias"])
    qe = relu(conv1d_same(q, W["query_proj.0.conv.weight"], W["query_proj.0.conv.bias"]))
    qe = relu(conv1d_same(qe, W["query_proj.2.conv.weight"], W["query_proj.2.conv.bias"]))
    qe = conv1d_same(qe, W["query_proj.4.conv.weight"], W["query_proj.4.conv.bias"])
    B, T, L = q.shape[0], q.shape[2], k.shape[2]
    a = np.empty((B, T, L), dtype)
    for b in range(B):
        d = (qe[b][:, :, None] - ke[b][:, None, :]) ** 2          # [n_att, T, L], one utterance at a time
        a[b] = dtype(-temperature) * d.sum(0)
    if prior is not None:
        a = log_softmax(a) + np.log(np.asarray(prior).astype(dtype) + dtype(1e-8))
    logprob = a.copy()
    if txt_lens is not None:
        for b in range(B):
            a[b, :, int(txt_lens[b]):] = -np.inf
    m = a.max(-1, keepdims=True)
    e = np.exp(a - m)
    return (e / e.sum(-1, keepdims=True)).astype(dtype), logprob


def mas_loops(frames_by_phonemes, log_map=False):
    """The search as two plain loops over (frame, phoneme), in this project's own terms: `best[p]` is the score of the best monotonic path that
    ends in phoneme p at the current frame, `stepped[t, p]` says whether that path entered (t, p) from phoneme p - 1.  What the fixtures of
    the reference's search pin: fp32 log (log 0 = -inf); frame 0 may only sit on phoneme 0; a step is preferred on a tie (>=, -inf ties
    included); the walk back starts at the last phoneme of the last frame; and cell (0, 0) is marked whatever the walk found in frame 0.
    log_map: the input already holds logarithms."""
    n_frames, n_phonemes = frames_by_phonemes.shape
    with np.errstate(divide="ignore"):
        score = np.array(frames_by_phonemes, copy=True) if log_map else np.log(frames_by_phonemes)
    minus_inf = score.dtype.type(-np.inf)
    best = np.full(n_phonemes, minus_inf, score.dtype)
    best[0] = score[0, 0]
    stepped = np.zeros((n_frames, n_phonemes), bool)
    for t in range(1, n_frames):
        nxt = np.empty_like(best)
        for p in range(n_phonemes):
            carry = best[p]
            if p > 0 and best[p - 1] >= carry:
                carry = best[p - 1]
                stepped[t, p] = True
            nxt[p] = score[t, p] + carry
        best = nxt
    marks = np.zeros_like(frames_by_phonemes)
    p = n_phonemes - 1
    for t in range(n_frames - 1, 0, -1):
        marks[t, p] = 1
        p -= int(stepped[t, p])
    marks[0, p] = 1
    marks[0, 0] = 1
    return marks


def mas_rows(attn_map, log_map=False):
    """mas_loops with each frame's columns at once: the same float32 additions and >= comparisons, hence the same path."""
    m, n = attn_map.shape
    with np.errstate(divide="ignore"):
        a = attn_map.copy() if log_map else np.log(attn_map)
    a[0, 1:] = -np.inf
    prev = a[0].copy()
    diag = np.zeros((m, n), bool)
    for i in range(1, m):
        left = np.concatenate([[-np.inf], prev[:-1]]).astype(a.dtype)
        d = left >= prev
        d[0] = False
        diag[i] = d
        prev = a[i] + np.where(d, left, prev)
    opt = np.zeros_like(attn_map)
    j = n - 1
    for i in range(m - 1, 0, -1):
        opt[i, j] = 1
        if diag[i, j]:
            j -= 1
    opt[0, j] = 1
    opt[0, 0] = 1
    return opt


def b_mas(b_attn_map, in_lens, out_lens, log_map=False, search=mas_loops):
    """The search per row on its slice [:out_lens[b], :in_lens[b]] of a [B, T, L] batch; zeros outside the slice."""
    out = np.zeros_like(b_attn_map)
    for b in range(b_attn_map.shape[0]):
        out[b, :out_lens[b], :in_lens[b]] = search(b_attn_map[b, :out_lens[b], :in_lens[b]], log_map)
    return out


def beta_binomial_prior(n_phonemes, n_frames, scale=1.0):
    """[n_frames, n_phonemes] float64: entry (t, p) is the beta-binomial pmf with n = n_phonemes trials and shape parameters
    (scale * (t + 1), scale * (n_frames - t)) at p -- the mass drifts from the first phoneme to the last as t runs over the frames.  (The
    distribution lives on 0 .. n_phonemes; only 0 .. n_phonemes - 1 is evaluated, so a row does not sum to 1: the fixtures pin that.)"""
    from scipy.stats import betabinom
    out = np.empty((n_frames, n_phonemes))
    phonemes = np.arange(n_phonemes)
    for t in range(n_frames):
        out[t] = betabinom.pmf(phonemes, n_phonemes, scale * (t + 1), scale * (n_frames - t))
    return out


def pad_prior(priors, max_mel_len, max_txt_len):
    out = np.zeros((len(priors), max_mel_len, max_txt_len), np.float32)
    for b, p in enumerate(priors):
        out[b, :p.shape[0], :p.shape[1]] = p
    return out


def valid_stats(x, ref, txt_lens, mel_lens, full_columns=False):
    """(mean, max) of |x - ref| over rows < mel_lens[b] and columns < txt_lens[b] (every column with full_columns)."""
    d = []
    for b in range(x.shape[0]):
        n = x.shape[2] if full_columns else int(txt_lens[b])
        d.append(np.abs(x[b, :int(mel_lens[b]), :n].astype(np.float64) - ref[b, :int(mel_lens[b]), :n].astype(np.float64)).ravel())
    d = np.concatenate(d)
    return float(d.mean()), float(d.max())


# ---------------------------------------------------------------- the attention pass alone (aln_attn_kernel through e2ealign_debug_attention)
U = 2.0 ** -24               # unit roundoff of float32
K_ULP = 4                    # assumed maximum ulp error of expf / logf on the device (tests/small_ref.py's K; assumed, not measured)
EPS_PRIOR = np.float32(1e-8)
SECOND_ORDER = 1.001         # the bars below are first-order in U; every relative error involved is below 1e-4, so 1 + 1e-3 covers the rest
ATTN_LDS_MAX = 64 * 1024


def attn_lds_bytes(TI, L, C):
    """aligner.hip: the LDS tile of the attention pass with TI frames per workgroup."""
    return (TI * C + 64 * (C | 1) + TI * L) * 4


def attn_frames_per_workgroup(L, C):
    """16 (four frames per wave) while that tile fits the LDS limit, else 4; None where not even 4 fit (refused)."""
    return 16 if attn_lds_bytes(16, L, C) <= ATTN_LDS_MAX else 4 if attn_lds_bytes(4, L, C) <= ATTN_LDS_MAX else None


def _lens_or_full(txt_lens, B, L):
    return np.full(B, L, np.int64) if txt_lens is None else np.asarray(txt_lens, np.int64)


def attention64(q, k, temperature, txt_lens=None, prior=None):
    """The attention pass in float64 on float32 inputs: q [B, T, C], k [B, L, C] -> (attn, attn_logprob, bar_attn, bar_logprob), all [B, T, L].

    The bars bound |float32 kernel - this| per element to first order in U = 2^-24, from the operations on the element's path:
      score    s = -temperature * sum_c (q - k)^2: one subtraction (relative U on the difference, 2 U on its square), a chain of ceil(C / 4)
               fused accumulations, two additions joining the four chains, one product; every term is >= 0, so the relative errors add:
               |ds| <= (ceil(C / 4) + 5) U |s|.  Without a prior attn_logprob = s.
      prior    x = s - m (U |x|; m is ANY common shift: log-softmax does not depend on it), ls = logf(sum expf(x)): the terms carry
               ds + U |x| + 2 K U (K ulp = K 2^-23 relative), weighted in the sum by their softmax weights w; the sum itself ceil(L / 64) + 6
               additions of positive terms (per-lane strided partial sums, then a 6-stage butterfly); logf adds 2 K U |ls|.  Then
               (x - ls) [U |x - ls|], logf(prior + 1e-8f) [the addition: U relative on the argument = U absolute on the logarithm; logf:
               2 K U |log|], and the last addition [U |attn_logprob|].
      softmax  over the valid keys, on the attn_logprob values v (error bl): y = v - m2 (U |y|), expf (2 K U), the sum (ceil(len / 64) + 6) U
               + the weighted errors of its terms, one division (U): relative to attn.  Masked keys are exactly 0 (bar 0).
    K = 4 is small_ref.py's allowance: assumed, not measured.  The whole bar is multiplied by SECOND_ORDER; 2^-149 is added to attn's for
    a result in the subnormals."""
    q64, k64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(k, np.float32).astype(np.float64)
    B, T, C = q64.shape
    L = k64.shape[1]
    t = np.float64(np.float32(temperature))
    d = ((q64[:, :, None, :] - k64[:, None, :, :]) ** 2).sum(-1)
    s = -t * d
    bs = (-(-C // 4) + 5) * U * np.abs(s)
    if prior is None:
        logp, bl = s, bs
    else:
        m = s.max(-1, keepdims=True)
        x = s - m
        e = np.exp(x)
        w = e / e.sum(-1, keepdims=True)
        ls = np.log(e.sum(-1, keepdims=True))
        lp = np.log(np.asarray(prior, np.float32).astype(np.float64) + np.float64(EPS_PRIOR))
        logp = (x - ls) + lp
        e_ls = (w * (bs + U * np.abs(x) + 2 * K_ULP * U)).sum(-1, keepdims=True) + (-(-L // 64) + 6) * U + 2 * K_ULP * U * np.abs(ls)
        bl = bs + U * np.abs(x) + e_ls + U * np.abs(x - ls) + U + 2 * K_ULP * U * np.abs(lp) + U * np.abs(logp)
    lens = _lens_or_full(txt_lens, B, L)
    attn, ba = np.zeros_like(logp), np.zeros_like(logp)
    for b in range(B):
        n = int(lens[b])
        v = logp[b, :, :n]
        y = v - v.max(-1, keepdims=True)
        e = np.exp(y)
        a = e / e.sum(-1, keepdims=True)
        term = bl[b, :, :n] + U * np.abs(y) + 2 * K_ULP * U
        rel = term + (a * term).sum(-1, keepdims=True) + (-(-n // 64) + 6) * U + U
        attn[b, :, :n] = a
        ba[b, :, :n] = rel * a * SECOND_ORDER + 2.0 ** -149
    return attn, logp, ba, bl * SECOND_ORDER


def _wave_reduce(per_lane, op):
    """The 6-stage xor butterfly over 64 lanes ([..., 64] float32): every lane ends with the same value."""
    v = per_lane
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., idx ^ o])
    return v[..., 0]


def _lane_partials(x, fill, op):
    """[..., n] float32 -> [..., 64]: lane l folds columns l, l + 64, ... in ascending order, starting from `fill`."""
    n = x.shape[-1]
    acc = np.full(x.shape[:-1] + (64,), fill, np.float32)
    for j0 in range(0, n, 64):
        blk = x[..., j0:j0 + 64]
        acc[..., :blk.shape[-1]] = op(acc[..., :blk.shape[-1]], blk)
    return acc


def attention32_kernel_order(q, k, temperature, txt_lens=None, prior=None, mut=None):
    """The attention pass in float32 in aln_attn_kernel's order: channel c goes to chain c mod 4 by one fused multiply-add (the product
    exact in float64, the sum rounded to float64 and then to float32: a double rounding, which can differ from the device's single one in
    rare last bits), chains joined (0 + 1) + (2 + 3), times -temperature; per row 64-lane strided partial maxima and sums, then the xor
    butterfly; numpy's float32 exp and log for expf and logf.  -> (attn, attn_logprob) float32.

    mut: one of the mutations the tests must catch -- "tail" (the last of the C mod 4 channels dropped), "stale" (a partial key tile keeps
    the previous tile's keys), "prior_len" (the prior's log-softmax over len instead of L), "softmax_L" (the masked softmax over L),
    "mask+1" (one masked key let in), "no_eps" (log(prior) without + 1e-8), "skip_last" (frame T - 1 of a partial frame tile not written)."""
    f32 = np.float32
    q, k = np.asarray(q, f32), np.asarray(k, f32)
    B, T, C = q.shape
    L = k.shape[1]
    if mut == "stale" and L % 64:
        k = k.copy()
        j0 = L // 64 * 64
        if j0:
            k[:, j0:] = k[:, j0 - 64:L - 64]
    acc = np.zeros((4, B, T, L), f32)
    for c in range(C - 1 if (mut == "tail" and C % 4) else C):
        dd = (q[:, :, None, c] - k[:, None, :, c]).astype(np.float64)
        acc[c & 3] = (dd * dd + acc[c & 3].astype(np.float64)).astype(f32)
    row = f32(-f32(temperature)) * ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    lens = _lens_or_full(txt_lens, B, L)
    with np.errstate(divide="ignore", invalid="ignore"):
        if prior is not None:
            pr = np.asarray(prior, f32)
            out = np.empty_like(row)
            for b in range(B):
                n = int(lens[b]) if mut == "prior_len" else L
                r = row[b]
                m = _wave_reduce(_lane_partials(r[:, :n], -np.inf, np.maximum), np.maximum)[:, None]
                ssum = _wave_reduce(_lane_partials(np.exp(r[:, :n] - m), 0.0, np.add), np.add)[:, None]
                out[b] = ((r - m) - np.log(ssum)) + np.log(pr[b] if mut == "no_eps" else pr[b] + EPS_PRIOR)
            row = out
        attn = np.zeros_like(row)
        for b in range(B):
            n = L if mut == "softmax_L" else min(L, int(lens[b]) + 1) if mut == "mask+1" else int(lens[b])
            v = row[b, :, :n]
            m2 = _wave_reduce(_lane_partials(v, -np.inf, np.maximum), np.maximum)[:, None]
            e = np.exp(v - m2)
            s2 = _wave_reduce(_lane_partials(e, 0.0, np.add), np.add)[:, None]
            attn[b, :, :n] = e / s2
    logp = row.copy()
    if mut == "skip_last" and T % 16:
        attn[:, T - 1], logp[:, T - 1] = np.nan, np.nan        # whatever the buffer held: the tests pre-fill with NaN
    return attn, logp
