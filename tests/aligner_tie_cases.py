"""Maps on which the monotonic search meets ties at every step, for tests/test_gpu_aligner_ties.py and tests/test_aligner_ties_host.py.

The wide search cases of tests/test_gpu_aligner.py use `random ** 6` and real attention maps: float ties do not occur there, so the
reference's `>=` rule (a tie, -inf ties included, takes the diagonal) is pinned by one 9 x 9 fixture on the one-column-per-lane form.  Here
every value comes from a set whose partial sums are exact in float32, so ties are the norm and the restatement is exact:
    log4    log map, values in {0, -1, -2, -3}
    loginf  log map, values in {0, -1, -inf}, with one whole -inf column and one whole -inf frame per row where the row has room
    prob01  probability map, values in {0, 1}: the device's logf and numpy's log agree exactly (0 and -inf)
Widths: every columns-per-lane form of the one-wavefront kernel (L <= 64, <= 128, <= 256), every 32-column back-pointer word boundary, and
two and three columns per thread of the workgroup form (L > 256, > 512).  Frames: around the 8-frame register block, and L + 9: with fewer
frames than phonemes the walk back runs down the diagonal through cells that are all -inf (row 0 is -inf past column 0), so only a map
with more frames than phonemes puts FINITE ties on the path at every column, lane boundary and back-pointer word."""
from __future__ import annotations

import numpy as np

import aligner_ref as ar
from kernel_ref import rng_of

f32 = np.float32
KINDS = ["log4", "loginf", "prob01"]
WIDTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513]
FRAMES = [1, 2, 8, 9, 10, 17]


def frames_of(L):
    return FRAMES + [L + 9]


# one tie map per back-pointer placement that needs the workspace (the bits no longer fit LDS): (B, T, L)
WORKSPACE_CASES = [(1, 5200, 64), (1, 1100, 257)]


def form_of(L):
    """Which kernel form a width takes: columns per lane of the one-wavefront kernel, or 0 for the workgroup kernel."""
    return 1 if L <= 64 else 2 if L <= 128 else 4 if L <= 256 else 0


def tie_map(kind, B, T, L):
    r = rng_of(f"tie_{kind}_{B}_{T}_{L}")
    if kind == "log4":
        return -r.integers(0, 4, (B, T, L)).astype(f32)
    if kind == "loginf":
        a = np.array([0.0, -1.0, -np.inf], f32)[r.integers(0, 3, (B, T, L))]
        for b in range(B):
            if L > 2:
                a[b, :, r.integers(1, L - 1)] = -np.inf
            if T > 2:
                a[b, r.integers(1, T - 1), :] = -np.inf
        return a
    assert kind == "prob01"
    return (r.random((B, T, L)) < 0.7).astype(f32)


def lens_of(T, L):
    """Row 0 whole, row 1 ragged in both lengths, row 2 with fewer frames than phonemes wherever L > 1 (the reference's closing opt[0, 0])."""
    il = np.array([L, max(1, L - 1 - L // 3), L], np.int64)
    ol = np.array([T, max(1, T - 1), max(1, min(T // 2, L - 1))], np.int64)
    return il, ol


def search(attn_map, log_map=False, strict=False, blind=0):
    """aligner_ref.mas_rows with two switches for the mutations.  strict: `>` in place of `>=`.  blind = c: the left neighbour of columns
    c, 2 c, ... (a lane's first column when a lane owns c columns) is taken as -inf, as if it did not arrive from the lane before."""
    m, n = attn_map.shape
    with np.errstate(divide="ignore"):
        a = attn_map.copy() if log_map else np.log(attn_map)
    a[0, 1:] = -np.inf
    prev = a[0].copy()
    diag = np.zeros((m, n), bool)
    for i in range(1, m):
        left = np.concatenate([[-np.inf], prev[:-1]]).astype(a.dtype)
        if blind:
            left[blind::blind] = -np.inf
        d = left > prev if strict else left >= prev
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


def want_of(kind, a, il, ol, **kw):
    return ar.b_mas(a, il, ol, log_map=kind != "prob01", search=lambda x, lm: search(x, lm, **kw))
