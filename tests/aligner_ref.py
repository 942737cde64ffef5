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
