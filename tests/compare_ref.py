"""A float64 restatement of include/e2etts_compare.h, independent of the library: cepstra, local cost, the DTW search with its tie
order, back-pointers and per-decision margins, the path and the figures along it.  The band predicate alone is not restated: it lives
once, in e2e_tts_amd/csrc/compare/plan.h, and is taken from there (tests/csrc/compare_plan_shim.cc, built with g++ at first use)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)
_SHIM = None


def shim():
    global _SHIM
    if _SHIM is None:
        d = tempfile.mkdtemp(prefix="e2ecmp_shim_")
        so = os.path.join(d, "libcompare_plan_shim.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "csrc", "compare_plan_shim.cc"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.e2ecmp_shim_band_mask.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p]
        lib.e2ecmp_shim_band_mask.restype = None
        lib.e2ecmp_shim_bp_words.argtypes = [C.c_longlong, C.c_longlong]
        lib.e2ecmp_shim_bp_words.restype = C.c_longlong
        lib.e2ecmp_shim_swapped.argtypes = [C.c_longlong, C.c_longlong]
        _SHIM = lib
    return _SHIM


def band_mask(Ta, Tb, band):
    """[Ta, Tb] bool: plan.h's band_allows on every cell (band < 0: all True)."""
    out = np.zeros((int(Ta), int(Tb)), np.uint8)
    shim().e2ecmp_shim_band_mask(int(Ta), int(Tb), int(band), out.ctypes.data)
    return out.astype(bool)


def dct_basis(n_mel, n_cep):
    """Rows 1 .. n_cep of the orthonormal DCT-II in float64."""
    k, m = np.arange(n_mel, dtype=np.float64)[:, None], np.arange(n_mel, dtype=np.float64)[None, :]
    c = np.sqrt(2.0 / n_mel) * np.cos(np.pi * (m + 0.5) * k / n_mel)
    c[0] = np.sqrt(1.0 / n_mel)
    return c[1:n_cep + 1]


def cepstra(mel, basis):
    """mel [T, n_mel], basis [n_cep, n_mel], both float32 -> (c [T, n_cep] float64, bar [T, n_cep]): the exact sum of the float32
    products (a product of two float32 is exact in float64; the float64 sum of n_mel of them is exact to 2^-53 relative, nothing beside
    the bar) and the bar the way tests/kernel_ref.py derives its bars: a chain of n_mel fp32 roundings, each at most 2^-24 of the
    running sum, which sum |terms| bounds: n_mel * 2^-24 * sum_m |basis[k, m] * mel[t, m]|."""
    m64, b64 = np.asarray(mel, np.float32).astype(np.float64), np.asarray(basis, np.float32).astype(np.float64)
    terms = m64[:, None, :] * b64[None, :, :]
    return terms.sum(-1), mel.shape[-1] * 2.0 ** -24 * np.abs(terms).sum(-1)


def cost_matrix(a, b):
    """d [Ta, Tb] float64 of float32 features a [Ta, D], b [Tb, D]: an explicit loop over k, the product and the sum rounded separately
    (numpy's sum is pairwise and is not this definition)."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    acc = np.zeros((a64.shape[0], b64.shape[0]), np.float64)
    for k in range(a64.shape[1]):
        diff = a64[:, k][:, None] - b64[:, k][None, :]
        prod = diff * diff
        acc = acc + prod
    return np.sqrt(acc)


def search(d, band=-1):
    """The definition's recurrence on a cost matrix, one anti-diagonal at a time -> dict: "D" [Ta, Tb] (inf outside the band and where
    nothing leads), "code" [Ta, Tb] int8 (0 diagonal, 1 (i-1, j), 2 (i, j-1)), "margin" [Ta, Tb] (second-best predecessor minus best:
    inf where only one exists, 0 at an exact tie), "status", and, with a path, "path" [N, 2] int32 in path order, "dist_total",
    "path_margin" (the smallest margin of the decisions on the path)."""
    Ta, Tb = d.shape
    allowed = band_mask(Ta, Tb, band)
    Dp = np.full((Ta + 1, Tb + 1), np.inf)          # Dp[i + 1, j + 1] = D(i, j)
    code = np.zeros((Ta, Tb), np.int8)
    margin = np.full((Ta, Tb), np.inf)
    Dp[1, 1] = d[0, 0] if allowed[0, 0] else np.inf
    for s in range(1, Ta + Tb - 1):
        i = np.arange(max(0, s - Tb + 1), min(Ta, s + 1))
        j = s - i
        diag, up, left = Dp[i, j], Dp[i, j + 1], Dp[i + 1, j]
        best, c = diag.copy(), np.zeros(i.size, np.int8)
        m = up < best
        best, c = np.where(m, up, best), np.where(m, 1, c)
        m = left < best
        best, c = np.where(m, left, best), np.where(m, 2, c)
        trio = np.sort(np.stack([diag, up, left]), 0)
        with np.errstate(invalid="ignore"):
            mg = trio[1] - trio[0]
        margin[i, j] = np.where(np.isfinite(trio[1]), mg, np.inf)
        code[i, j] = c
        Dp[i + 1, j + 1] = np.where(allowed[i, j], d[i, j] + best, np.inf)
    D = Dp[1:, 1:]
    r = {"D": D, "code": code, "margin": margin, "status": 0 if np.isfinite(D[-1, -1]) else 1}
    if r["status"]:
        return r
    i, j, cells, pm = Ta - 1, Tb - 1, [], np.inf
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            break
        pm = min(pm, margin[i, j])
        c = code[i, j]
        i, j = (i - 1, j) if c == 1 else (i, j - 1) if c == 2 else (i - 1, j - 1)
    r["path"] = np.array(cells[::-1], np.int32)
    r["dist_total"] = float(D[-1, -1])
    r["path_margin"] = float(pm)
    return r


def sync_path(Ta, Tb):
    n = min(int(Ta), int(Tb))
    return np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)


def brute_force(d):
    """The smallest total over every monotone path of steps (1, 1), (1, 0), (0, 1) from (0, 0) to the end, by enumeration."""
    Ta, Tb = d.shape

    def go(i, j):
        if i == Ta - 1 and j == Tb - 1:
            return d[i, j]
        best = np.inf
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Ta and j + dj < Tb:
                best = min(best, go(i + di, j + dj))
        return d[i, j] + best
    return go(0, 0)


def figures(path, d, mel_a=None, mel_b=None, f0_a=None, f0_b=None, dist_total=None):
    """The fields of e2ecmp_result along a path, in float64."""
    i, j = path[:, 0], path[:, 1]
    N = len(path)
    dp = d[i, j]
    r = {"n_path": N, "status": 0, "dist_total": float(dp.sum()) if dist_total is None else float(dist_total), "mcd_db": float(MCD_SCALE * (dp.sum() / N)),
         "mel_l1": np.nan, "f0_rmse_hz": np.nan, "f0_rmse_cents": np.nan, "n_voiced_both": 0, "n_vuv_mismatch": 0}
    if mel_a is not None and mel_b is not None:
        r["mel_l1"] = float(np.abs(np.asarray(mel_a, np.float32).astype(np.float64)[i] - np.asarray(mel_b, np.float32).astype(np.float64)[j]).sum() / (N * mel_a.shape[1]))
    if f0_a is not None and f0_b is not None:
        x, y = np.asarray(f0_a, np.float32).astype(np.float64)[i], np.asarray(f0_b, np.float32).astype(np.float64)[j]
        va, vb = x > 0, y > 0
        both = va & vb
        r["n_voiced_both"], r["n_vuv_mismatch"] = int(both.sum()), int((va != vb).sum())
        if both.any():
            r["f0_rmse_hz"] = float(np.sqrt(((y[both] - x[both]) ** 2).sum() / both.sum()))
            r["f0_rmse_cents"] = float(np.sqrt(((1200.0 * np.log2(y[both] / x[both])) ** 2).sum() / both.sum()))
    return r


def no_path():
    nan = float("nan")
    return {"n_path": 0, "status": 1, "dist_total": nan, "mcd_db": nan, "mel_l1": nan, "f0_rmse_hz": nan, "f0_rmse_cents": nan, "n_voiced_both": 0, "n_vuv_mismatch": 0}


def compare(a, b, mode="dtw", band=-1, mel_a=None, mel_b=None, f0_a=None, f0_b=None):
    """One pair, whole: features a [Ta, D], b [Tb, D] float32 -> (figures dict with "path", the search's dict or None for "sync")."""
    d = cost_matrix(a, b)
    if mode == "sync":
        path = sync_path(len(a), len(b))
        r = figures(path, d, mel_a, mel_b, f0_a, f0_b)
        r["path"] = path
        return r, None
    s = search(d, band)
    if s["status"]:
        r = no_path()
        r["path"] = np.zeros((0, 2), np.int32)
        return r, s
    r = figures(s["path"], d, mel_a, mel_b, f0_a, f0_b, s["dist_total"])
    r["path"] = s["path"]
    return r, s
