"""The case matrix and the check functions of tests/test_gpu_aligner_attention.py (aln_attn_kernel alone, through the test build's
e2ealign_debug_attention) and tests/test_aligner_attention_host.py, which runs the same checks on the CPU restatements and their mutations.

Shapes (B <= 3, T <= 40): n_att 1 .. 8 (the C mod 4 channel tail), 80, 127, 128; L 1, 63, 64, 65, 130 (the 64-key tile and its tail); T 1, 15,
16, 17, 33 (the 16-frame tile and the per-wave break); two shapes past the 64 KiB tile of 16 frames, which take the 4-frame instantiation.
Two tiers:
  exact    q, k multiples of 2^-4 in [-4, 4], temperature 2^-11, no prior: every squared distance is an integer multiple of 2^-8 below
           2^24 of them in ANY summation order, so attn_logprob must equal the numpy value bit for bit, padded key columns included;
  general  Gaussian q, k, both temperatures, no prior / the beta-binomial prior / a uniform random prior, every txt_lens mode: per element
           under aligner_ref.attention64's bar, and the aggregate 4 x the float32 restatement's own mean deviation from 512 elements up."""
from __future__ import annotations

import numpy as np

import aligner_ref as ar
from kernel_ref import rng_of

f32 = np.float32
T_EXACT = 2.0 ** -11
TEMPS = [T_EXACT, 5e-4]
LENS_MODES = ["absent", "full", "ragged", "one"]
PRIORS = ["none", "betabinom", "uniform"]
AGG_MIN, AGG_FACTOR = 512, 4.0

# (n_att, L, T)
SHAPES = ([(A, 65, 17) for A in (1, 2, 3, 4, 5, 6, 7, 8, 80, 127, 128)] + [(8, L, 17) for L in (1, 63, 64, 130)]
          + [(6, 65, T) for T in (1, 15, 16, 33)])
FOUR_FRAME_SHAPES = [(4, 1040, 5), (127, 400, 6)]
CROSS_SHAPE = (6, 65, 17)          # every (txt_lens mode, prior, temperature) combination runs at this shape


def lens_of(mode, B, L):
    if mode == "absent":
        return None
    if mode == "full":
        return np.full(B, L, np.int64)
    if mode == "one":
        return np.ones(B, np.int64)
    return np.array([L, max(1, (2 * L) // 3), max(1, L // 2 - 1)], np.int64)[:B]


def exact_inputs(A, L, T, identical=False):
    """Multiples of 2^-4 in [-4, 4].  identical: within each row every key equals the first, so every valid score of a frame is the same."""
    r = rng_of(f"attn_exact_{A}_{L}_{T}")
    q = (r.integers(-64, 65, (3, T, A)) / 16).astype(f32)
    k = (r.integers(-64, 65, (3, L, A)) / 16).astype(f32)
    if identical:
        k[:] = k[:, :1]
    return q, k


def exact_want(q, k):
    """attn_logprob of the exact tier, with the proof that it is exact: 2^8 d is an integer below 2^24."""
    d = ((q.astype(np.float64)[:, :, None, :] - k.astype(np.float64)[:, None, :, :]) ** 2).sum(-1)
    assert np.all(d * 256 == np.round(d * 256)) and d.max() * 256 < 2 ** 24 and q.shape[2] * 64 * 256 <= 2 ** 21
    return f32(-T_EXACT) * d.astype(f32)


def general_inputs(A, L, T, lens_mode, prior_kind):
    r = rng_of(f"attn_gen_{A}_{L}_{T}")
    B = 3
    q, k = r.standard_normal((B, T, A)).astype(f32), r.standard_normal((B, L, A)).astype(f32)
    lens = lens_of(lens_mode, B, L)
    prior = None
    if prior_kind == "betabinom":       # per row over its own phonemes, zero-padded: what the data pipeline hands the model
        n = ar._lens_or_full(lens, B, L)
        prior = ar.pad_prior([ar.beta_binomial_prior(int(n[b]), T) for b in range(B)], T, L)
    elif prior_kind == "uniform":
        prior = r.random((B, T, L)).astype(f32)
    return q, k, lens, prior


def general_cases():
    """(A, L, T, lens_mode, prior_kind, temperature): the full cross at CROSS_SHAPE; elsewhere every prior, the modes and temperatures in turn."""
    out = []
    for i, (A, L, T) in enumerate(SHAPES + FOUR_FRAME_SHAPES):
        if (A, L, T) == CROSS_SHAPE:
            out += [(A, L, T, m, p, t) for m in LENS_MODES for p in PRIORS for t in TEMPS]
        else:
            out += [(A, L, T, LENS_MODES[(i + j) % 4], p, TEMPS[(i + j) % 2]) for j, p in enumerate(PRIORS)]
    return out


# ---------------------------------------------------------------- the checks (the GPU test's and the mutations')
def check_masked(attn, lens):
    """attn is exactly 0 on masked keys."""
    if lens is None:
        return []
    return [f"row {b}: attn not exactly 0 on masked keys" for b in range(attn.shape[0]) if np.any(attn[b, :, int(lens[b]):] != 0)]


def check_exact(attn, logp, q, k, lens, identical=False):
    """Exact tier: attn_logprob bit for bit on every column; attn 0 on masked keys, inside the bar elsewhere, and exactly fl(1 / len) on the
    valid keys where they are identical."""
    fails = check_masked(attn, lens)
    want = exact_want(q, k)
    nd = int((np.ascontiguousarray(logp).view(np.uint32) != want.view(np.uint32)).sum()) if not np.isnan(logp).any() else int(np.isnan(logp).sum())
    if nd:
        fails.append(f"attn_logprob differs from the exact value on {nd} of {want.size} elements")
    a64, _, ba, _ = ar.attention64(q, k, T_EXACT, lens, None)
    if not np.all(np.abs(attn - a64) <= ba):
        fails.append("attn outside the bar")
    if identical:
        n = ar._lens_or_full(lens, attn.shape[0], attn.shape[2])
        for b in range(attn.shape[0]):
            if np.any(attn[b, :, :int(n[b])] != f32(1) / f32(n[b])):
                fails.append(f"row {b}: attn is not fl(1 / len) on identical keys")
    return fails, nd


def check_general(attn, logp, ref, yard=None):
    """ref: aligner_ref.attention64's tuple.  Per element under the bar; with `yard` (the float32 restatement's (attn, attn_logprob)) and at
    least AGG_MIN elements, the mean deviation within AGG_FACTOR x the restatement's own.  -> (fails, figures)."""
    a64, l64, ba, bl = ref
    fails, fig = [], {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, got, want, bar in (("attn", attn, a64, ba), ("attn_logprob", logp, l64, bl)):
            err = np.abs(got.astype(np.float64) - want)
            bad = ~(err <= bar)                                     # a NaN fails
            ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
            fig[name] = float(np.nanmax(ratio)) if not np.isnan(got).any() else float("inf")
            if bad.any():
                fails.append(f"{name}: {int(bad.sum())} of {bad.size} elements outside the bar (worst ratio {fig[name]:.3g})")
            if yard is not None and got.size >= AGG_MIN:
                own = float(np.abs(yard[0 if name == "attn" else 1].astype(np.float64) - want).mean())
                mean = float(err.mean())
                fig[name + "_agg"] = mean / own if own > 0 else (0.0 if mean == 0 else float("inf"))
                if not mean <= AGG_FACTOR * own:
                    fails.append(f"{name}: mean deviation {mean:.3e} above {AGG_FACTOR:g} x the float32 restatement's {own:.3e}")
    return fails, fig
