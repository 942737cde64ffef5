"""The beta-binomial attention prior of include/e2etts_align.h restated in float64 numpy through log-gamma terms (scipy.special.gammaln),
independent of scipy.stats.betabinom.pmf, which e2e_tts_amd.aligner.batch_prior -- the reference's own path -- calls; the criterion
``check_prior`` that the restatement, its mutations and the device (tests/test_gpu_aligner_prior.py) are held to; and the mutations.

Criterion.  ``want`` is batch_prior's float32 tensor.  Where want >= 2^-126 the bit patterns differ by at most 1 fp32 ulp: a float64
value whose relative error is far below 2^-24 (measured: 1.4e-11 at most) rounds to want or to a neighbour.  Where want < 2^-126 the
result may be the subnormal or 0: 0 <= got <= 2^-126.  The padded region is exactly 0.  At most 0.1 % of the normal-range elements of a
case differ at all (the restatement differs from scipy on 0 elements for every shape up to 700 x 760)."""
from __future__ import annotations

import numpy as np

F32_MIN_NORMAL = np.float32(2.0 ** -126)
MAX_ULP = 1
MAX_SHARE = 1e-3

MUTATIONS = ["n_minus_1", "zero_based_frame", "swapped", "beta_off_by_one", "scaling_alpha_only", "outcome_P_stored", "float32_logs"]


def prior64(P: int, M: int, s: float = 1.0, mutation: str | None = None) -> np.ndarray:
    """[M, P] float64 (``outcome_P_stored``: [M, P + 1]): frame t (0-based), phoneme k holds
    C(n, k) B(k + a, n - k + b) / B(a, b) with n = P, a = s (t + 1), b = s (M - t)."""
    from scipy.special import gammaln
    assert mutation is None or mutation in MUTATIONS
    dt = np.float32 if mutation == "float32_logs" else np.float64
    lg = (lambda x: gammaln(np.asarray(x, dt)).astype(dt)) if dt is np.float32 else gammaln
    n = dt(P - 1 if mutation == "n_minus_1" else P)
    t = np.arange(M, dtype=dt)[:, None]
    k = np.arange(P + 1 if mutation == "outcome_P_stored" else P, dtype=dt)[None, :]
    i = t if mutation == "zero_based_frame" else t + 1           # the reference counts frames from 1
    a, b = dt(s) * i, dt(s) * (dt(M) - t)
    if mutation == "beta_off_by_one":
        b = dt(s) * (dt(M) - i)
    if mutation == "scaling_alpha_only":
        b = dt(M) - t
    if mutation == "swapped":
        a, b = b, a
    with np.errstate(divide="ignore", invalid="ignore"):
        log = (lg(n + 1) - lg(k + 1) - lg(n - k + 1)) + (lg(k + a) + lg(n - k + b)) - lg(n + a + b) - (lg(a) + lg(b) - lg(a + b))
        return np.exp(log.astype(np.float64))


def batch64(txt_lens, mel_lens, T: int, L: int, s: float = 1.0, mutation: str | None = None) -> np.ndarray:
    """The padded [B, T, L] float32 batch: zeros assigned over, float64 rounded to fp32 once."""
    out = np.zeros((len(txt_lens), int(T), int(L)), np.float32)
    for b, (P, M) in enumerate(zip(txt_lens, mel_lens)):
        p = prior64(int(P), int(M), s, mutation)
        out[b, :p.shape[0], :p.shape[1]] = p
    return out


def _ulps(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """|difference of the bit patterns| of non-negative fp32 values (for them the patterns are ordered as the values are)."""
    return np.abs(np.ascontiguousarray(got, np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(want, np.float32).view(np.int32).astype(np.int64))


def check_prior(got, want, txt_lens, mel_lens):
    """-> (fails, figures): ``fails`` is empty when ``got`` meets the criterion of the module docstring against ``want``."""
    got, want = np.asarray(got), np.asarray(want)
    fails, fig = [], {"share": 0.0, "max_ulp": 0, "normal": 0}
    if got.shape != want.shape or got.dtype != np.float32:
        return [f"shape / dtype {got.shape} {got.dtype}, expected {want.shape} float32"], fig
    valid = np.zeros(want.shape, bool)
    for b, (P, M) in enumerate(zip(txt_lens, mel_lens)):
        valid[b, :int(M), :int(P)] = True
    if np.isnan(got).any():
        return [f"{int(np.isnan(got).sum())} NaN"], fig
    pad_bits = np.ascontiguousarray(got).view(np.uint32)[~valid]
    if pad_bits.any():
        fails.append(f"padded region: {int((pad_bits != 0).sum())} elements are not exactly 0")
    normal = valid & (want >= F32_MIN_NORMAL)
    small = valid & ~normal
    if small.any() and not ((got[small] >= 0) & (got[small] <= F32_MIN_NORMAL)).all():
        fails.append("below the normal range: a value outside [0, 2^-126]")
    if normal.any():
        u = _ulps(got[normal], want[normal])
        if (got[normal] < 0).any():
            fails.append("a negative value")
        fig.update(share=float((u != 0).mean()), max_ulp=int(u.max()), normal=int(normal.sum()))
        if fig["max_ulp"] > MAX_ULP:
            fails.append(f"{int((u > MAX_ULP).sum())} of {u.size} normal-range elements off by more than {MAX_ULP} ulp (worst {fig['max_ulp']})")
        if fig["share"] > MAX_SHARE:
            fails.append(f"{fig['share']:.3%} of the normal-range elements differ (at most {MAX_SHARE:.1%})")
    return fails, fig
