"""The cases of tests/test_gpu_fastformer_kernels.py, their inputs, their references (computed once per case and shared) and the check
functions that judge a kernel's `out` and workspace -- imported by the GPU module and by tests/test_fastformer_kernel_ref_host.py, which runs
mutated restatements through the same checks.

A case is a dict: name, B, N, H, hs, pad (v_ld = H + pad), scale (bool), lens (list or None), kind ("gauss" | "rising" | "uniform" |
"two_level"), want (what ff_shape must say: (rp, maxt), asserted)."""
from __future__ import annotations

import functools
import zlib

import numpy as np

import fastformer_kernel_ref as fr

f32, f64 = np.float32, np.float64


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ragged_lens(B, N):
    """Every kind of row: whole, empty, half, above N, negative, one, N - 1, ..."""
    pool = [N, 0, N // 2, N + 5, -3, 1, max(N - 1, 0), (2 * N) // 3]
    return [pool[b % len(pool)] for b in range(B)]


def _case(name, B, N, H, hs, want, pad=0, scale=False, lens="ragged", kind="gauss"):
    return dict(name=name, B=B, N=N, H=H, hs=hs, pad=pad, scale=scale, lens=ragged_lens(B, N) if lens == "ragged" else lens, kind=kind, want=want)


def _both(name, *a, **kw):
    return [_case(name, *a, **kw), _case(name + "_scale", *a, scale=True, **kw)]


# The smallest shapes that reach each instantiation (want = (RP, the workgroup size it is compiled for)) and each path.  Aggregate rule: B x H >= 512.
GENERAL = (
    _both("rp4_h8_hs1_n33", 64, 33, 8, 1, (4, 512), pad=4)
    + _both("rp4_h24_hs2_n17", 3, 17, 24, 2, (4, 512))                      # 12 heads: 48 of 64 threads live
    + _both("rp4_h64_hs8_n15", 8, 15, 64, 8, (4, 512), pad=8)
    + _both("rp4_h16_hs4_n16", 5, 16, 16, 4, (4, 512))
    + _both("rp4_h8_hs2_n1", 3, 1, 8, 2, (4, 512), lens=[1, 0, 7])         # runs of a single row
    + _both("rp4_1024_h384_hs2_n33", 2, 33, 384, 2, (4, 1024), lens=[33, 20])   # the shipped size: 192 heads, 768 threads
    + _both("rp2_h8_hs1_bn8192", 64, 128, 8, 1, (2, 512), pad=4)
    + _both("rp2_1024_h512_hs1_n33", 1, 33, 512, 1, (2, 1024), lens=[21])   # 512 heads, LDS exactly 64 KiB
    + _both("rp1_h1024_hs2_n33", 1, 33, 1024, 2, (1, 512), lens=[12])
    + [_case("rp1_h768_hs2_n17", 1, 17, 768, 2, (1, 512), lens=None, scale=True),     # 384 threads
       _case("rp1_h1024_hs8_n16", 1, 16, 1024, 8, (1, 512), lens=[9]),                 # 128 threads
       _case("multi_tile_n16385", 1, 16385, 8, 2, (2, 512), lens=[9000], scale=True),  # 1025 tiles: 513 runs of two tiles, the last of one row
       _case("multi_tile_rising", 1, 16385, 8, 2, (2, 512), lens=None, kind="rising")])
UNIFORM = [_case("u_h8_hs1_n33", 8, 33, 8, 1, (4, 512), pad=4, kind="uniform", scale=True),
           _case("u_h24_hs2_n17", 8, 17, 24, 2, (4, 512), kind="uniform"),
           _case("u_h8_hs4_n16_null", 3, 16, 8, 4, (4, 512), kind="uniform", lens=None),
           _case("u_h512_hs1_n17", 2, 17, 512, 1, (2, 1024), kind="uniform", lens=[5, 17]),
           _case("u_h1024_hs8_n16", 2, 16, 1024, 8, (1, 512), kind="uniform", lens=[16, 3], scale=True),
           _case("u_multi_tile", 1, 16385, 8, 2, (2, 512), kind="uniform", lens=[7001])]
TWO_LEVEL = [_case("t_h8_hs1_n33", 8, 33, 8, 1, (4, 512), kind="two_level", pad=4),
             _case("t_h24_hs2_n17", 8, 17, 24, 2, (4, 512), kind="two_level", scale=True),
             _case("t_h64_hs8_n31", 3, 31, 64, 8, (4, 512), kind="two_level", lens=[0, 0, 0]),
             _case("t_h768_hs2_n17", 1, 17, 768, 2, (1, 512), kind="two_level", lens=[4])]
ALL = {c["name"]: c for c in GENERAL + UNIFORM + TWO_LEVEL}
# RP = 4 against RP = 2: the same 600 rows once alone and once as row RP_ROW of a batch of 14 (14 x 600 >= 8192)
RP_N, RP_H, RP_HS, RP_B, RP_ROW = 600, 64, 2, 14, 5


def dyadic(r, shape, lo=-8, hi=8, unit=2.0 ** -3):
    return (r.integers(lo, hi + 1, shape) * unit).astype(f32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(v [B, N, H], scale [B, H] or None, wl_t [H, heads] (the logit weights transposed), bl [heads], lens)."""
    c = ALL[name]
    B, N, H, hs = c["B"], c["N"], c["H"], c["hs"]
    NH = H // hs
    r = rng_of("ffk_" + name)
    kind = c["kind"]
    if kind in ("gauss", "rising"):
        v = r.standard_normal((B, N, H)).astype(f32)
        wl_t = (r.standard_normal((H, NH)) / np.sqrt(H)).astype(f32)
        bl = r.standard_normal(NH).astype(f32)
        scale = r.standard_normal((B, H)).astype(f32) if c["scale"] else None
        if kind == "rising":                     # every head's logit climbs by about 100 over the sequence, 0.2 per two-tile run: the running maximum rises from tile to tile
            wl_t = np.abs(wl_t) + f32(0.25)
            v = (f32(0.1) * v + (f32(32.0) * np.arange(N, dtype=f32) / f32(N))[None, :, None]).astype(f32)
    elif kind == "uniform":                      # wl = 0: every logit is fl(bias / div) (+ the shift), whatever v holds
        v = dyadic(r, (B, N, H))
        wl_t = np.zeros((H, NH), f32)
        bl = (r.standard_normal(NH) + 0.5).astype(f32)
        bl[bl == 0] = f32(0.375)
        scale = (r.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (B, H))).astype(f32) if c["scale"] else None
    else:                                        # two_level: the last four channels decide; channel H - 4 + (n mod 4) of a rejected row holds -1024
        v = dyadic(r, (B, N, H))
        scale = (r.choice([0.5, 1.0, 2.0], (B, H))).astype(f32) if c["scale"] else None
        wl_t = np.zeros((H, NH), f32)
        for j in range(4):
            wl_t[H - 4 + j] = 1 + (j + np.arange(NH)) % 4
        bl = np.zeros(NH, f32)
        sel = r.random((B, N)) < 0.4
        sel[:, N - 1] = True                     # the last row (of a partial tile when N % 16 != 0) is always selected
        v[:, :, H - 4:] = 0
        for b in range(B):
            rej = np.flatnonzero(~sel[b])
            v[b, rej, H - 4 + rej % 4] = -1024.0
        v[:, N - 1, :H - 4] += f32(3.0)          # and stands out: leaving it out moves every mean
    return dict(v=v, scale=scale, wl_t=wl_t, bl=bl, lens=c["lens"])


def selected_rows(c, d):
    """[B, N] bool: the rows whose weight is exactly 1 / count in an exact-tier case (all others exactly 0)."""
    B, N, H = d["v"].shape
    len_ = fr.clamp_lens(d["lens"], B, N)
    padded = np.arange(N)[None, :] >= len_[:, None]
    base = np.ones((B, N), bool) if c["kind"] == "uniform" else ~(d["v"][:, :, H - 4:] != 0).any(-1)
    sel = base & padded
    none = ~sel.any(1)                           # no padded candidate: the shifted rows compete among themselves
    sel[none] = base[none]
    return sel


def exactness(name):
    """The conditions the exact tier rests on, asserted on the CPU: every sum of v' over any subset of rows is a float32 in any order
    (max sum |v'| / unit < 2^24), the selected and the rejected logits are what the tier says, and some row is selected in every batch row."""
    c, d = ALL[name], inputs(name)
    vp = fr.scaled_values(d["v"], d["scale"])
    assert np.array_equal(vp.astype(f64), d["v"].astype(f64) * (1 if d["scale"] is None else d["scale"].astype(f64)[:, None, :]))   # the product is exact
    assert np.all(vp.astype(f64) / 2.0 ** -7 == np.round(vp.astype(f64) / 2.0 ** -7))         # all on the 2^-7 grid
    assert np.abs(vp).astype(f64).sum(1).max() / 2.0 ** -7 < 2 ** 24
    s = fr.logits_f32(d["v"], d["scale"], d["wl_t"], d["bl"], d["lens"], c["hs"])
    sel = selected_rows(c, d)
    assert sel.any(1).all()
    top = s.max(-1, keepdims=True)
    on = np.broadcast_to(sel[:, None, :], s.shape)
    assert np.all(s[on].reshape(-1) == np.broadcast_to(top, s.shape)[on].reshape(-1))        # selected rows: exactly the maximum
    assert np.all((s - top)[~on] <= -200.0)                                                   # all others: expf(s - max) == 0
    fr.exp_facts()
    return True


def exact_out(name):
    """out [B, H] = fl(sum over the selected rows of v' / their count): one rounding, the sum and the count being exact."""
    c, d = ALL[name], inputs(name)
    vp = fr.scaled_values(d["v"], d["scale"]).astype(f64)
    sel = selected_rows(c, d)
    return (((vp * sel[:, :, None]).sum(1) + 0.0) / sel.sum(1)[:, None]).astype(f32)      # (+ 0.0: the kernel's sums start from +0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything a case is judged against, computed once: the launch shape, the restated logits, their run maxima, the float64 pool and
    its bar, the float32 yardstick (general tier) or the exact output (exact tier)."""
    c, d = ALL[name], inputs(name)
    B, N, H, hs = c["B"], c["N"], c["H"], c["hs"]
    sh = fr.ff_shape(B, N, H, hs)
    vp = fr.scaled_values(d["v"], d["scale"])
    s = fr.logits_f32(d["v"], d["scale"], d["wl_t"], d["bl"], d["lens"], hs)
    ref = dict(case=c, sh=sh, vp=vp, s=s, runmax=fr.run_maxima(s, N, sh))
    if c["kind"] in ("gauss", "rising"):
        ref["out64"], ref["S"], _ = fr.pool64(s, vp, hs)
        ref["bar"] = fr.pool_bar(s, vp, hs, sh)
        ref["yard"], ref["yard_ws"] = fr.pool_f32(s, vp, hs, sh)
    else:
        ref["exact"] = exact_out(name)
    return ref


def simulate(name, mut=None):
    """(out, ws) of the float32 restatement in the kernel's order, with a mutation of the logits or of the pool."""
    c, d = ALL[name], inputs(name)
    sh = fr.ff_shape(c["B"], c["N"], c["H"], c["hs"])
    ref = reference(name)
    if mut in LOGIT_MUTATIONS:
        s = fr.logits_f32(d["v"], d["scale"], d["wl_t"], d["bl"], d["lens"], c["hs"], mut)
        return fr.pool_f32(s, ref["vp"], c["hs"], sh)
    zero_logit = (d["bl"] / f32(np.sqrt(f64(c["hs"])))).astype(f32)       # fl(fl(0 + bias) / div) + 0
    return fr.pool_f32(ref["s"], ref["vp"], c["hs"], sh, mut, zero_logit)


LOGIT_MUTATIONS = ("mask_not_inverted", "mask_off_by_one", "div_after_shift", "scale_not_in_logits", "drop_last_group", "ksplit4")
POOL_MUTATIONS = ("stale_rows", "no_rescale", "merge_without_maxima", "drop_last_run", "head_plus_one")


# ---------------------------------------------------------------- the checks (failures as a list of strings, figures as a dict)
def check_shape(ref, splits, ws_bytes):
    """The restated launch shape against the case's target and the library's two queries."""
    c, sh = ref["case"], ref["sh"]
    fails = []
    if (sh["rp"], sh["maxt"]) != tuple(c["want"]):
        fails.append(f"{c['name']}: the restated ff_shape gives RP {sh['rp']} / {sh['maxt']} threads, the case is meant for {c['want']}")
    if splits != sh["splits"] or ws_bytes != fr.workspace_bytes(c["B"], c["N"], c["H"], c["hs"]):
        fails.append(f"{c['name']}: the library reports {splits} splits / {ws_bytes} bytes, the restatement {sh['splits']} / {fr.workspace_bytes(c['B'], c['N'], c['H'], c['hs'])}")
    return fails


def check_workspace(ref, ws):
    """Bit for bit: the max entry of every (b, run, head) is the largest restated logit of the run; in runs of a single row the sum is 1 and
    the weighted sums are the (scaled) row."""
    c, sh = ref["case"], ref["sh"]
    ws = np.asarray(ws, f32).reshape(c["B"], sh["splits"], sh["heads"], c["hs"] + 2)
    fails = []
    nd = fr.diff_count(ws[..., 0], ref["runmax"])
    if nd:
        fails.append(f"{c['name']}: {nd} of {ref['runmax'].size} run maxima differ from the restated logits")
    for sp, (a, b) in enumerate(fr.run_bounds(c["N"], sh)):
        if b - a == 1:
            row = ref["vp"][:, a].reshape(c["B"], sh["heads"], c["hs"]) + f32(0.0)     # fmaf(1, row, +0): a -0 comes out as +0
            if fr.diff_count(ws[:, sp, :, 1], np.ones((c["B"], sh["heads"]), f32)) or fr.diff_count(ws[:, sp, :, 2:], row):
                fails.append(f"{c['name']}: run {sp} of one row does not hold (1, the row)")
    return fails, dict(maxima=int(ref["runmax"].size), maxima_differing=nd)


def check_exact(ref, out):
    c = ref["case"]
    nd = fr.diff_count(np.asarray(out, f32).reshape(ref["exact"].shape), ref["exact"])
    return ([f"{c['name']}: {nd} of {ref['exact'].size} outputs differ from the exact mean"] if nd else []), dict(elements=int(ref["exact"].size), differing=nd)


def check_general(ref, out):
    """Per element under the derived bar; for cases of at least AGG_MIN_ELEMS outputs the mean deviation at most AGG_FACTOR x the yardstick's."""
    c = ref["case"]
    out = np.asarray(out, f32).astype(f64).reshape(ref["out64"].shape)
    fails = []
    if not np.all(np.isfinite(out)):
        return [f"{c['name']}: non-finite outputs"], dict(worst=np.inf, agg=None, elements=int(out.size))
    err = np.abs(out - ref["out64"])
    worst = float((err / ref["bar"]).max())
    if worst > 1:
        fails.append(f"{c['name']}: worst error / bar {worst:.3g} ({int((err > ref['bar']).sum())} of {err.size} elements above the bar)")
    agg = None
    if out.size >= fr.AGG_MIN_ELEMS:
        yard = float(np.abs(ref["yard"].astype(f64) - ref["out64"]).mean())
        agg = float(err.mean()) / (fr.AGG_FACTOR * yard)
        if agg > 1:
            fails.append(f"{c['name']}: mean deviation {err.mean():.3g} above {fr.AGG_FACTOR:g} x the float32 yardstick's {yard:.3g}")
    return fails, dict(worst=worst, agg=agg, elements=int(out.size))


# ---------------------------------------------------------------- ff_scale
SCALE_CASES = [  # (name, B, N, H, q_ld)
    ("h4", 2, 5, 4, 4), ("h4_wide", 3, 7, 4, 8), ("total_4096", 1, 64, 64, 64), ("total_4096_wide", 2, 32, 64, 128),
    ("total_1032", 1, 43, 24, 24), ("total_1032_wide", 1, 43, 24, 48), ("two_blocks_and_a_bit", 3, 61, 12, 24)]
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.17549435e-38, np.inf, -np.inf, 3.4028235e38, -3.4028235e38, 1.0, -1.5], f32)


def scale_inputs(name):
    _, B, N, H, q_ld = next(c for c in SCALE_CASES if c[0] == name)
    r = rng_of("ffs_" + name)
    q, x, gk = r.standard_normal((B, N, H)).astype(f32), r.standard_normal((B, N, H)).astype(f32), r.standard_normal((B, H)).astype(f32)
    k = min(q.size // 2, 4 * SPECIALS.size)                  # signed zeros, subnormals, infinities, the largest finite numbers
    for arr in (q, x):
        arr.reshape(-1)[r.choice(arr.size, k, replace=False)] = r.choice(SPECIALS, k)
    gk.reshape(-1)[r.choice(gk.size, min(gk.size // 2, 6), replace=False)] = r.choice(SPECIALS, min(gk.size // 2, 6))
    return q, gk, x


def check_scale(name, wv, qx):
    q, gk, x = scale_inputs(name)
    want_wv, want_qx = fr.scale_f32(q, gk, x)
    n1, n2 = fr.diff_count(np.asarray(wv).reshape(q.shape), want_wv), fr.diff_count(np.asarray(qx).reshape(q.shape), want_qx)
    return ([f"ff_scale {name}: {n1} wv and {n2} qx elements of {q.size} differ"] if n1 or n2 else []), dict(elements=2 * int(q.size), differing=n1 + n2)
