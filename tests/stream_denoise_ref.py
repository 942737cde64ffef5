"""Numpy restatement of the denoised vocoder stream (include/e2etts.h: e2etts_vocoder_stream_begin_denoised; engine.hip:
e2etts_vocoder_stream_push; engine_denoise.hip: denoise_stream_impl), for the host tests.

``stream_plan``      the window arithmetic of _push, in mel frames: what each push's window holds and which of its frames it emits.
``denoise_window``   the denoiser as a function of one window of a longer signal, in ``denoiser_ref.denoise_rows``' arithmetic (float32 rows of
                     hop samples, one product per tap): an edge that is a real end of the signal is reflected, an edge that is context is
                     copied, frames stay on the signal's absolute hop grid, and the envelope counts the absolute frames covering a sample.
``denoise_stream``   both together on a signal that stands in for the vocoder's output (the vocoder itself is a function of the window
                     with halo H; here the samples are simply given).
"""
from __future__ import annotations

import numpy as np

from denoiser_ref import _subtract


def stream_plan(chunks, H):
    """chunks: frames per push (the last one closes the stream); H: frames of context per side (vocoder halo + denoiser delay).
    Yields per push: (abs0, total, left_ctx, emit_end, n_emit, last) -- the window holds the absolute frames abs0 .. abs0 + total - 1 and
    emits its frames left_ctx .. emit_end - 1."""
    carry_n = emitted = abs0 = 0
    for i, n in enumerate(chunks):
        last = i == len(chunks) - 1
        total = carry_n + n
        left_ctx = min(H, emitted, carry_n)
        emit_end = total if last else total - H
        n_emit = max(0, emit_end - left_ctx)
        keep_from = max(0, (emit_end if n_emit > 0 else left_ctx) - H)
        yield abs0, total, left_ctx, emit_end, n_emit, last
        carry_n = 0 if last else total - keep_from
        abs0 += keep_from
        emitted += n_emit


def envelope_at(win_sq, p, hop, n_frames=None):
    """librosa's window_sumsquare at the absolute padded positions p: a float32 accumulator over the frames covering each, in ascending
    order; frames 0 .. n_frames - 1 exist (None: the signal's end is not known, and far away)."""
    N = len(win_sq)
    p = np.asarray(p, np.int64)
    f_lo = np.where(p - N + 1 <= 0, 0, (p - N + hop) // hop)
    f_hi = p // hop
    if n_frames is not None:
        f_hi = np.minimum(f_hi, n_frames - 1)
    env = np.zeros(len(p), np.float32)
    for k in range(N // hop + 1):
        f = f_lo + k
        ok = f <= f_hi
        env[ok] = (env[ok].astype(np.float64) + win_sq[p[ok] - f[ok] * hop]).astype(np.float32)
    return env


def denoise_window(seg, S0, right_real, e0, n_out, bias, strength, fwd, inv, win_sq, hop):
    """seg: the samples S0 .. S0 + L - 1 of the signal (its start iff S0 == 0, its end included iff right_real) -> the denoised samples
    seg[e0 : e0 + n_out]."""
    N = fwd.shape[1]
    V, bins, half = N // hop, N // 2 + 1, N // 2
    seg = np.asarray(seg, np.float32)
    L = len(seg)
    left_real = S0 == 0
    if left_real and right_real and L <= half:
        return seg[e0:e0 + n_out].copy()
    lead = half if left_real else 0
    p = seg
    if left_real:
        p = np.concatenate([seg[1:half + 1][::-1], p])
    if right_real:
        p = np.concatenate([p, seg[-half - 1:-1][::-1]])
    R = len(p) // hop
    G = R - V + 1
    rows = p.reshape(R, hop)
    spec = np.zeros((G, N + 2), np.float32)
    for j in range(V):
        spec += rows[j:j + G] @ fwd[:, j * hop:(j + 1) * hop].T
    spec = _subtract(spec, np.asarray(bias), strength, bins)
    z = np.zeros((V - 1, N + 2), np.float32)
    padded = np.concatenate([z, spec, z])      # at a context edge the frames beyond are missing: the rows they spoil are not emitted
    out = np.zeros((R, hop), np.float32)
    for j in range(V):
        k = V - 1 - j
        out += padded[j:j + R] @ inv[:, k * hop:(k + 1) * hop]
    y = out.reshape(-1)[e0 + lead:e0 + lead + n_out].copy()
    pos = S0 + e0 + half + np.arange(n_out, dtype=np.int64)
    env = envelope_at(win_sq, pos, hop, (S0 + L) // hop + 1 if right_real else None)
    ok = env > np.finfo(np.float32).tiny
    y[ok] = y[ok] / env[ok]
    y *= np.float32(N / hop)
    return y


def denoise_stream(x, chunks, halo, delay, hop_length, bias, strength, fwd, inv, win_sq, hop):
    """x [T * hop_length]: the whole (vocoder) waveform; chunks: frames per push.  Returns the emitted pieces, and per push (frames pushed so
    far, frames emitted so far)."""
    pieces, lag, pushed, emitted = [], [], 0, 0
    for (abs0, total, left_ctx, emit_end, n_emit, last), n in zip(stream_plan(chunks, halo + delay), chunks):
        pushed += n
        if n_emit > 0:
            d_lo, d_hi = max(0, left_ctx - delay), min(total, emit_end + delay)
            S0 = (abs0 + d_lo) * hop_length
            seg = x[S0:(abs0 + d_hi) * hop_length]
            assert (abs0 + d_hi) * hop_length <= len(x)
            pieces.append(denoise_window(seg, S0, last, (left_ctx - d_lo) * hop_length, n_emit * hop_length, bias, strength, fwd, inv, win_sq, hop))
            emitted += n_emit
        lag.append((pushed, emitted))
    return pieces, lag
