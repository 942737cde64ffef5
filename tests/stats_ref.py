"""A numpy restatement of the corpus-statistics library, written from include/e2etts_stats.h in the header's order of operations, with
float32 where the header says float32 and float64 elsewhere; and the bars of the tests with their derivation.

``mut`` arguments are the mutations tests/test_stats_host.py shows the checks to catch: "closed_fences" (a fence comparison made
non-strict), "fma_lerp" (the multiply and add of the percentile AND of the fences fused: computed in float64 and rounded once), "drop_one"
(one kept value dropped), "sample_std" (n - 1 in the variance).  For q = 25 and 75 the lerp's own product is exact -- gamma and 1 - gamma
are 0, 1/4 or 1/2 there -- so fusing it changes no bit; the product 1.5 * iqr of the fences is not exact, and that is where contraction
shows.

Bars (derived, not measured; u = 2^-53, the unit roundoff of a double).
  sum     A sum of N doubles in any order is within (N - 1) u sum|x| of the exact sum (Higham, Accuracy and Stability of Numerical
          Algorithms, eq. 4.4, to first order).
  mean    Two such sums in different orders, one division each: relative bar 4 N u sum|x| / |sum x|.  The factor 4 covers that BOTH sides
          carry the error (2 x) and the reference's own different summation order -- pairwise in numpy, Chan merges per file in sklearn --
          whose merge steps add an operation or two per element (2 x).
  var     M2 = sum (x - m)^2 is a sum of N non-negative terms: (N - 1) u from the summation, 3 u from each term's subtraction and square;
          an error dm of the mean enters M2 only in second order (N dm^2, since sum (x - m) = 0).  That is (N + 2) u relative for the
          two-pass form about the exact mean.  The merged form adds d^2 na nb / n terms whose d = mean_b - mean_a carries the means'
          ABSOLUTE error, of the order u |mean|, against a spread of the order of the standard deviation: the conditioning factor
          1 + mean^2 / var (Chan, Golub and LeVeque 1983, section 3).  Relative bar of the variance: 4 (N + 2) u (1 + mean^2 / var).
  std     sqrt halves a relative error and adds one rounding: var_bar / 2 + 2 u.
  min/max z = (double(raw) - mean) / std with raw exact: |dz| <= |mean| mean_bar / std + |z| (std_bar + 2 u).
N is the count the figure is over (a row's kept count, the corpus's kept count).  Nothing discrete is compared under a tolerance:
percentiles, fences, counts and raw min / max are exact."""
import math

import numpy as np

U = 2.0 ** -53
F0, ENERGY, PITCH = 0, 1, 2
f32 = np.float32


def vindex(n: int, q: int):
    """(lo, hi, gamma) of the header: v = (n - 1) q / 100 in double, gamma rounded to float32."""
    v = (n - 1) * (q / 100.0)
    lo = int(math.floor(v))
    return lo, min(lo + 1, n - 1), f32(v - lo)


def lerp(a, b, g, mut=None):
    a, b, g = f32(a), f32(b), f32(g)
    d = f32(b - a)
    if mut == "fma_lerp":   # one rounding for multiply and add
        if g < f32(0.5):
            return f32(np.float64(a) + np.float64(d) * np.float64(g))
        return f32(np.float64(b) - np.float64(d) * np.float64(f32(f32(1.0) - g)))
    if g < f32(0.5):
        return f32(a + f32(d * g))
    return f32(b - f32(d * f32(f32(1.0) - g)))


def fences(row, mut=None):
    """-> (sorted row, p25, p75, lower, upper) in float32."""
    s = np.sort(np.asarray(row, dtype=np.float32))
    n = len(s)
    p = []
    for q in (25, 75):
        lo, hi, g = vindex(n, q)
        p.append(lerp(s[lo], s[hi], g, mut))
    p25, p75 = p
    if mut == "fma_lerp":   # p25 - 1.5 * iqr and p75 + 1.5 * iqr as one fused operation each, which is what contraction makes of them
        iqr = np.float64(f32(p75 - p25))
        return s, p25, p75, f32(np.float64(p25) - 1.5 * iqr), f32(np.float64(p75) + 1.5 * iqr)
    spread = f32(f32(1.5) * f32(p75 - p25))
    return s, p25, p75, f32(p25 - spread), f32(p75 + spread)


def _sums(kept):
    """sum, mean, m2 of float32 values in double; the sums exactly rounded (math.fsum), so the bars need not cover this side's order."""
    x = np.asarray(kept, dtype=np.float64)
    if x.size == 0:
        return 0.0, 0.0, 0.0
    total = math.fsum(x)
    mean = total / x.size
    return total, mean, math.fsum((x - mean) * (x - mean))


def row_record(row, kind=ENERGY, mut=None) -> dict:
    """One row's record (the fields of e2est_row)."""
    row = np.asarray(row, dtype=np.float32)
    if not np.isfinite(row).all():
        return {"n": len(row), "status": 1}
    if kind == F0:
        kept = row[row != 0]
        total, mean, m2 = _sums(kept)
        return dict(n=len(row), n_kept=len(kept), sum=total, mean=mean, m2=m2, p25=f32(0), p75=f32(0), lower=f32(0), upper=f32(0), min=f32(0), max=f32(0),
                    status=0, kept=kept)
    s, p25, p75, lower, upper = fences(row, mut)
    with np.errstate(invalid="ignore"):
        keep = (s >= lower) & (s <= upper) if mut == "closed_fences" else (s > lower) & (s < upper)
    kept = s[keep]
    if mut == "drop_one" and len(kept) > 1:
        kept = kept[:-1]
    total, mean, m2 = _sums(kept)
    return dict(n=len(row), n_kept=len(kept), sum=total, mean=mean, m2=m2, p25=p25, p75=p75, lower=lower, upper=upper, min=s[0], max=s[-1], status=0, kept=kept)


def empty_acc() -> dict:
    return dict(rows=0, n_frames=0, n=0, mean=0.0, m2=0.0, rmin=f32(np.inf), rmax=f32(-np.inf))


def merge(acc: dict, rec: dict) -> dict:
    """Chan's update of the header, one row."""
    acc = dict(acc)
    acc["rows"] += 1
    acc["n_frames"] += rec["n"]
    acc["rmin"], acc["rmax"] = min(acc["rmin"], rec["min"]), max(acc["rmax"], rec["max"])
    nb = rec["n_kept"]
    if nb == 0:
        return acc
    if acc["n"] == 0:
        acc.update(n=nb, mean=rec["mean"], m2=rec["m2"])
        return acc
    na, nt = float(acc["n"]), float(acc["n"] + nb)
    d = rec["mean"] - acc["mean"]
    acc["mean"] = acc["mean"] + d * float(nb) / nt
    acc["m2"] = acc["m2"] + rec["m2"] + d * d * na * float(nb) / nt
    acc["n"] += nb
    return acc


def block(acc: dict, kind: int, mut=None) -> dict:
    """mean, std (and min, max of the normalised values) of an accumulator; raises where the header has an error."""
    if acc["n"] == 0:
        raise ValueError("nothing kept")
    n = acc["n"] - 1 if mut == "sample_std" else acc["n"]
    out = {"mean": float(acc["mean"]), "std": float(np.sqrt(acc["m2"] / n)), "n_kept": acc["n"]}
    if kind != F0:
        if acc["m2"] == 0.0:
            out["std"] = 1.0
        out["min"] = float((np.float64(acc["rmin"]) - out["mean"]) / out["std"])
        out["max"] = float((np.float64(acc["rmax"]) - out["mean"]) / out["std"])
    return out


def corpus(utts, mut=None, kinds=("f0", "energy", "pitch")) -> dict:
    """stats.json's dict of a corpus (tests/stats_cases.py: a list of utterances), rows merged in order, with the sums the bars need
    under "_bars": per kind (N, sum|x|, sum x) of the kept values."""
    out, bars = {}, {}
    for name in kinds:
        kind = {"f0": F0, "energy": ENERGY, "pitch": PITCH}[name]
        acc, kept = empty_acc(), []
        for u in utts:
            r = row_record(u[name], kind, mut)
            acc = merge(acc, r)
            kept.append(np.asarray(r["kept"], dtype=np.float64))
        out[name] = block(acc, kind, mut)
        k = np.concatenate(kept)
        bars[name] = (len(k), math.fsum(np.abs(k)), math.fsum(k))
    out["_bars"] = bars
    return out


def normalize(values, lens, mean: float, std: float) -> np.ndarray:
    """The data loader's target: float32 arithmetic, 0 beyond each length."""
    v = np.asarray(values, dtype=np.float32)
    out = np.zeros(v.shape, np.float32)
    for b, n in enumerate(np.asarray(lens).reshape(-1)):
        out[b, :n] = (v[b, :n] - f32(mean)) / f32(std)
    return out


# ---- the bars
def mean_bar(N: int, sum_abs: float, total: float) -> float:
    """relative"""
    return 4.0 * N * U * sum_abs / abs(total) if total != 0 else math.inf


def var_bar(N: int, mean: float, var: float) -> float:
    """relative"""
    return 4.0 * (N + 2) * U * (1.0 + mean * mean / var) if var > 0 else math.inf


def std_bar(N: int, mean: float, std: float) -> float:
    """relative"""
    return var_bar(N, mean, std * std) / 2.0 + 2.0 * U


def z_bar(z: float, N: int, sum_abs: float, total: float, mean: float, std: float) -> float:
    """absolute, of a normalised min or max"""
    return abs(mean) * mean_bar(N, sum_abs, total) / std + abs(z) * (std_bar(N, mean, std) + 2.0 * U)


def check_block(got: dict, want: dict, bars, scaled: bool) -> list:
    """The figures of ``got`` (a block of stats.json) against ``want`` under the bars -> a list of what fails (empty: passes).  A
    variance of exactly 0 (std 1 for a scaled kind, 0 for f0) is compared exactly."""
    N, sum_abs, total = bars
    bad = []
    m, s = want["mean"], want["std"]
    if not abs(got["mean"] - m) <= mean_bar(N, sum_abs, total) * abs(m):
        bad.append(("mean", got["mean"], m))
    exact_std = s == 0.0 or (scaled and s == 1.0 and got["std"] == 1.0)
    if exact_std:
        if got["std"] != s:
            bad.append(("std", got["std"], s))
        sb = 0.0
    else:
        sb = std_bar(N, m, s)
        if not abs(got["std"] - s) <= sb * s:
            bad.append(("std", got["std"], s))
    if scaled:
        for k in ("min", "max"):
            tol = abs(m) * mean_bar(N, sum_abs, total) / s + abs(want[k]) * (sb + 2.0 * U)
            if not abs(got[k] - want[k]) <= tol:
                bad.append((k, got[k], want[k]))
    return bad


def check_row(got: dict, want: dict) -> list:
    """A row's sum / mean / m2 against the restatement's exactly rounded ones under the bars (N = the row's kept count)."""
    bad = []
    N = int(want["n_kept"])
    if N == 0:
        return [(k, got[k]) for k in ("sum", "mean", "m2") if got[k] != 0.0]
    kept = np.asarray(want["kept"], dtype=np.float64)
    sum_abs = math.fsum(np.abs(kept))
    if not abs(got["sum"] - want["sum"]) <= (N - 1) * U * sum_abs + U * abs(want["sum"]):
        bad.append(("sum", got["sum"], want["sum"]))
    if want["sum"] != 0 and not abs(got["mean"] - want["mean"]) <= mean_bar(N, sum_abs, want["sum"]) * abs(want["mean"]):
        bad.append(("mean", got["mean"], want["mean"]))
    if want["m2"] == 0.0:
        if got["m2"] != 0.0:
            bad.append(("m2", got["m2"], 0.0))
    elif not abs(got["m2"] - want["m2"]) <= var_bar(N, want["mean"], want["m2"] / N) * want["m2"]:
        bad.append(("m2", got["m2"], want["m2"]))
    return bad
