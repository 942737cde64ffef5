"""CPU checks of what tests/test_gpu_fastformer_kernels.py relies on (tests/fastformer_kernel_ref.py, tests/fastformer_kernel_cases.py): the exact
fused multiply-add against rational arithmetic, the restated launch shape against the library's queries, the restated logits and the float64
pool against the oracle's FastAttention and against torch, the exactness conditions of the exact tier, the float32 restatement in the kernel's
order under every check, every listed mutation failing the GPU module's own check functions at the smallest case it exists in, and every
refusal of launch_ff_pool / launch_ff_scale (no GPU: a wrapper that refuses returns before it launches)."""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fastformer_kernel_cases as fc   # noqa: E402
import fastformer_kernel_ref as fr     # noqa: E402

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- the exact fused multiply-add
def _tie_triples(r, n):
    """Triples whose float64 sum a * b + c is INEXACT and rounds onto a float32 tie: c a float32 of [1, 2), a * b = -+ half an ulp of c times
    (1 - x^2 2^-46) -- (1 + x 2^-23)(1 - x 2^-23) -- so that the true sum lies 2^-70 x^2 inside the tie and float64 cannot see it."""
    x = r.integers(1, 256, n).astype(f64)
    a = (1.0 + x * 2.0 ** -23).astype(f32)
    sign = r.choice([-1.0, 1.0], n)
    b = (sign * (1.0 - x * 2.0 ** -23) * 2.0 ** -24).astype(f32)
    c = (1.0 + r.integers(0, 2 ** 23, n) * 2.0 ** -23).astype(f32)
    e = r.integers(-20, 20, n)                                        # the same at other exponents
    return a, (b * 2.0 ** e).astype(f32), (c * 2.0 ** e).astype(f32)


def test_fma32_is_the_rational_fma():
    """>= 1e5 triples against fmaf evaluated in Fractions: Gaussian triples, cancelling ones, subnormal results, exact ties, and triples
    constructed to sit on ties after the float64 rounding (the double-rounding case, which must take the rational path)."""
    r = fc.rng_of("fma32")
    n = 30000
    sets = []
    a, b = r.standard_normal(n).astype(f32), r.standard_normal(n).astype(f32)
    sets.append((a, b, r.standard_normal(n).astype(f32)))
    sets.append((a, b, (-(a.astype(f64) * b.astype(f64)) * (1 + r.integers(-3, 4, n) * 2.0 ** -23)).astype(f32)))        # cancellation
    sets.append(((a * f32(2.0 ** -70)).astype(f32), (b * f32(2.0 ** -65)).astype(f32), (r.standard_normal(n) * 2.0 ** -140).astype(f32)))   # subnormals
    k = r.integers(0, 2 ** 23, n)
    sets.append((np.full(n, 2.0 ** -12, f32), np.full(n, 2.0 ** -12, f32), (1.0 + k * 2.0 ** -23).astype(f32)))          # exact ties: c + half an ulp
    sets.append(_tie_triples(r, n))
    before = fr.FMA_STATS["rational"]
    total = 0
    for i, (a, b, c) in enumerate(sets):
        got = fr.fma32(a, b, c)
        want = np.array([fr.fma_fraction(x, y, z) for x, y, z in zip(a, b, c)], f32)
        assert fr.diff_count(got, want) == 0, i
        total += a.size
        if i == 4:                               # the constructed ties: the float64 shortcut is wrong on about half of them
            assert fr.FMA_STATS["rational"] - before >= n
            assert fr.diff_count(fr.fma32_once(a, b, c), want) > n // 4
        if i == 3:                               # exact ties go to even without the rational path
            assert fr.FMA_STATS["rational"] == before
            assert np.all(got.view(np.uint32) % 2 == 0)
    assert total >= 100000
    for x in (Fraction(1, 3), Fraction(-5, 7) * Fraction(2) ** -140, Fraction(2) ** -149, Fraction(3, 2) * Fraction(2) ** -149, Fraction(2 ** 24 + 1)):
        v = fr.round_fraction_f32(x)
        lo, hi = np.nextafter(v, f32(-np.inf)), np.nextafter(v, f32(np.inf))
        assert abs(Fraction(float(v)) - x) <= min(abs(Fraction(float(lo)) - x), abs(Fraction(float(hi)) - x))


# ---------------------------------------------------------------- the launch shape
def test_ff_shape_against_the_library():
    """Every case takes the instantiation it is meant for, all five are there, and the restated splits / workspace bytes are the library's
    over a sweep across every threshold (B x N = 8192, heads x RP = 1024, 64 KiB of LDS, 1024 tiles)."""
    import fastformer_harness as fh
    got = set()
    for c in fc.ALL.values():
        sh = fr.ff_shape(c["B"], c["N"], c["H"], c["hs"])
        assert (sh["rp"], sh["maxt"]) == tuple(c["want"]), c["name"]
        assert not fc.check_shape(dict(case=c, sh=sh), fh.splits(c["B"], c["N"], c["H"], c["hs"]), fh.workspace_bytes(c["B"], c["N"], c["H"], c["hs"]))
        got.add((sh["rp"], sh["maxt"]))
    assert got == {(4, 512), (4, 1024), (2, 512), (2, 1024), (1, 512)}
    sh = fr.ff_shape(1, 16385, 8, 2)
    assert (sh["rows_per_wg"], sh["splits"], sh["tiles_per_run"]) == (32, 513, 2) and fr.run_bounds(16385, sh)[-1] == (16384, 16385)
    assert fr.ff_shape(1, 33, 512, 1)["lds"] == 65536 and fr.ff_shape(1, 17, 768, 2)["threads"] == 384 and fr.ff_shape(1, 16, 1024, 8)["threads"] == 128
    assert fr.ff_shape(3, 17, 24, 2)["threads"] == 64 and fr.ff_shape(3, 17, 24, 2)["heads"] * 4 == 48
    n = 0
    for B in (1, 2, 14, 64, 1025):
        for N in (1, 15, 16, 17, 33, 127, 128, 600, 8191, 8192, 16384, 16385, 16401, 40000):
            for H, hs in ((4, 1), (8, 1), (8, 2), (24, 2), (64, 8), (256, 1), (260, 1), (384, 2), (512, 1), (516, 2), (768, 2), (1024, 2), (1024, 8), (1024, 4)):
                sh = fr.ff_shape(B, N, H, hs)
                assert fh.splits(B, N, H, hs) == sh["splits"] and fh.workspace_bytes(B, N, H, hs) == fr.workspace_bytes(B, N, H, hs), (B, N, H, hs)
                assert sh["threads"] <= 1024 and sh["lds"] <= 65536 and sh["rows_per_wg"] % 16 == 0 and (sh["splits"] - 1) * sh["rows_per_wg"] < N
                n += 1
    assert n == 5 * 14 * 14
    for bad in ((0, 5, 8, 1), (1, 0, 8, 1), (1, 5, 6, 1), (1, 5, 8, 3), (1, 5, 12, 8), (1, 5, 1024, 1), (65536, 5, 8, 1), (1, (1 << 24) + 1, 8, 1), (1, 5, 1028, 2)):
        assert fh.splits(*bad) == 0 and fh.workspace_bytes(*bad) == 0 and fr.ff_check(*bad) is not None, bad


# ---------------------------------------------------------------- the restatements against the oracle and torch
def _tiny():
    r = fc.rng_of("ffk_tiny")
    B, N, H, hs = 3, 7, 8, 2
    q, k = r.standard_normal((B, N, H)).astype(f32), r.standard_normal((B, N, H)).astype(f32)
    wq, wk = (r.standard_normal((H // hs, H)) / 3).astype(f32), (r.standard_normal((H // hs, H)) / 3).astype(f32)
    bq, bk = r.standard_normal(H // hs).astype(f32), r.standard_normal(H // hs).astype(f32)
    return B, N, H, hs, q, k, wq, wk, bq, bk, [N, 3, 0]


def _two_pools(B, N, H, hs, q, k, wq, wk, bq, bk, lens):
    sh = fr.ff_shape(B, N, H, hs)
    s_q = fr.logits_f32(q, None, wq.T.copy(), bq, lens, hs)
    gq, _, _ = fr.pool64(s_q, q, hs)
    gq32 = gq.astype(f32)
    s_k = fr.logits_f32(k, gq32, wk.T.copy(), bk, lens, hs)
    gk, _, _ = fr.pool64(s_k, fr.scaled_values(k, gq32), hs)
    return gq, gk, sh


# a row without padding has every logit shifted by -10000, i.e. rounded to the 2^-10 grid of float32 there, which a float64 evaluation does
# not do: the weights then agree to e^(2^-11) - 1 only.  Rows with padding put all their weight on unshifted logits.
TOL_GRID, TOL = 2e-3, 2e-6


def test_pools_against_the_oracles_fast_attention():
    """FastformerOracle.fast_attention in float64 with identity query / key / transform layers returns gk * q + q: both pools are in it."""
    from fastformer_ref import FastformerOracle
    B, N, H, hs, q, k, wq, wk, bq, bk, lens = _tiny()
    assert np.array_equal(q, k) is False
    o = object.__new__(FastformerOracle)
    eye, zero = np.eye(H), np.zeros(H)
    o.dt, o.n_head = f64, hs
    o.sd = {"a.query.weight": eye, "a.query.bias": zero, "a.key.weight": eye, "a.key.bias": zero, "a.transform.weight": eye, "a.transform.bias": zero,
            "a.to_q_attn_logits.weight": wq.astype(f64), "a.to_q_attn_logits.bias": bq.astype(f64),
            "a.to_k_attn_logits.weight": wq.astype(f64), "a.to_k_attn_logits.bias": bq.astype(f64)}
    pad = np.arange(N)[None, :] >= np.asarray(lens)[:, None]
    h = q.astype(f64)                                              # identity layers: q = k = h
    y = o.fast_attention("a", h, pad)
    gk_oracle = (y - h) / h                                        # y = gk (broadcast over n) * q + q
    gq, gk, _ = _two_pools(B, N, H, hs, q, q, wq, wq, bq, bq, lens)
    for b in range(B):
        tol = TOL_GRID if lens[b] >= N else TOL
        assert np.allclose(gk_oracle[b], gk[b][None, :], rtol=50 * tol, atol=50 * tol), b   # (two pools deep, divided by q: looser than below)


def test_pools_against_torch():
    """The reference's own lines (fastformer.py:223-259) in torch float64 on the CPU, pool by pool."""
    import torch
    B, N, H, hs, q, k, wq, wk, bq, bk, lens = _tiny()
    nh = H // hs
    tq, tk = torch.from_numpy(q).double(), torch.from_numpy(k).double()
    pad = torch.from_numpy(np.arange(N)[None, :] >= np.asarray(lens)[:, None])
    mask = ((1.0 - pad.double()) * -10000.0)[:, None, :]
    div = hs ** 0.5

    def pool(x, w, b):
        s = (torch.nn.functional.linear(x, torch.from_numpy(w).double(), torch.from_numpy(b).double()).transpose(1, 2) / div) + mask
        a = torch.softmax(s, -1)
        return torch.matmul(a.unsqueeze(2), x.view(B, N, nh, hs).transpose(1, 2)).transpose(1, 2).reshape(B, H)

    gq_t = pool(tq, wq, bq)
    gq, gk, _ = _two_pools(B, N, H, hs, q, k, wq, wk, bq, bk, lens)
    gk_t = pool(tk * torch.from_numpy(gq.astype(f32)).double()[:, None, :], wk, bk)
    for b in range(B):
        tol = TOL_GRID if lens[b] >= N else TOL
        assert np.allclose(gq_t[b].numpy(), gq[b], rtol=tol, atol=tol) and np.allclose(gk_t[b].numpy(), gk[b], rtol=tol, atol=tol), b
    # and the restated logits against a float64 evaluation: within an ulp of the float32 grid where they land
    s = fr.logits_f32(q, None, wq.T.copy(), bq, lens, hs)
    s64 = (q.astype(f64) @ wq.astype(f64).T + bq).transpose(0, 2, 1) / div + mask.numpy()
    assert np.all(np.abs(s - s64) <= 2 * np.spacing(np.abs(s).astype(f32)) + 1e-6)


# ---------------------------------------------------------------- the restatement under the GPU module's checks; the exactness conditions
def test_exact_tier_conditions_and_the_restatement():
    fr.exp_facts()
    for c in fc.UNIFORM + fc.TWO_LEVEL:
        assert fc.exactness(c["name"])
        out, ws = fc.simulate(c["name"])
        ref = fc.reference(c["name"])
        assert not fc.check_exact(ref, out)[0] and not fc.check_workspace(ref, ws)[0], c["name"]
    # the lens forms the issue lists are all there: N, 0, above N, negative, NULL
    lens = fc.ALL["u_h24_hs2_n17"]["lens"]
    assert {17, 0, 22, -3} <= set(lens) and fc.ALL["u_h8_hs4_n16_null"]["lens"] is None
    # two-level: every one of the last four channels rejects some row, and the last row is selected
    d = fc.inputs("t_h8_hs1_n33")
    assert all((d["v"][:, :, 8 - 4 + j] != 0).any() for j in range(4)) and fc.selected_rows(fc.ALL["t_h8_hs1_n33"], d)[:, -1].all()


def test_float32_restatement_stays_under_the_bar_at_every_case():
    worst = 0.0
    for c in fc.GENERAL:
        ref = fc.reference(c["name"])
        fails, fig = fc.check_general(ref, ref["yard"])
        assert not fails and not fc.check_workspace(ref, ref["yard_ws"])[0], (c["name"], fails)
        assert np.all(ref["bar"] > 0) and np.all(np.isfinite(ref["bar"]))
        worst = max(worst, fig["worst"])
    print(f"[fastformer kernels] float32 restatement in the kernel's order: worst error / bar {worst:.3f}")
    assert worst < 1
    # the rising case: the running maximum rises between the two tiles of most runs (the rescale is not 1)
    ref = fc.reference("multi_tile_rising")
    s = ref["s"][0]
    first, second = s[:, :16384].reshape(-1, 512, 2, 16)[:, :, 0].max(-1), s[:, :16384].reshape(-1, 512, 2, 16)[:, :, 1].max(-1)
    assert (second > first).mean() > 0.8 and ref["sh"]["tiles_per_run"] == 2


# ---------------------------------------------------------------- mutations, through the GPU module's own check functions
def _fails(name, mut):
    ref = fc.reference(name)
    out, ws = fc.simulate(name, mut)
    kind = fc.ALL[name]["kind"]
    f_out = fc.check_general(ref, out)[0] if kind in ("gauss", "rising") else fc.check_exact(ref, out)[0]
    return bool(f_out), bool(fc.check_workspace(ref, ws)[0])


def test_unmutated_restatement_passes_where_the_mutations_are_tried():
    for name in ("u_h24_hs2_n17", "rp4_h24_hs2_n17", "rp4_h24_hs2_n17_scale", "t_h8_hs1_n33", "rp4_h64_hs8_n15", "multi_tile_rising", "rp4_h8_hs1_n33"):
        assert _fails(name, None) == (False, False), name


def test_mutations_of_the_mask():
    assert _fails("u_h24_hs2_n17", "mask_not_inverted")[0] and _fails("rp4_h24_hs2_n17", "mask_not_inverted") == (True, True)
    assert _fails("u_h24_hs2_n17", "mask_off_by_one")[0] and _fails("rp4_h24_hs2_n17", "mask_off_by_one")[0]


def test_mutation_stale_rows_in_a_partial_tile():
    assert _fails("u_h24_hs2_n17", "stale_rows")[0] and _fails("rp4_h24_hs2_n17", "stale_rows")[0]
    assert _fails("u_h8_hs4_n16_null", "stale_rows") == (False, False)        # N = 16: no partial tile, the mutation does not exist


def test_mutations_of_the_chain():
    assert _fails("t_h8_hs1_n33", "drop_last_group")[0] and _fails("rp4_h24_hs2_n17", "drop_last_group") == (True, True)
    out_fails, ws_fails = _fails("rp4_h64_hs8_n15", "ksplit4")
    assert ws_fails                                                           # the bit-for-bit logit check sees a chain summed in another order
    print(f"[fastformer kernels] chain split four ways along K: fails the run maxima; fails the bar on out: {out_fails}")
    assert _fails("rp4_h24_hs2_n17_scale", "scale_not_in_logits") == (True, True)


def test_mutation_division_after_the_shift():
    assert any(_fails("rp4_h24_hs2_n17", "div_after_shift"))
    assert _fails("rp4_h24_hs2_n17", "div_after_shift")[1]
    assert _fails("rp4_h8_hs1_n33", "div_after_shift") == (False, False)      # head size 1: div = 1, provably the same computation


def test_mutations_of_the_running_state_and_the_merge():
    assert _fails("multi_tile_rising", "no_rescale")[0]
    assert _fails("rp4_h8_hs1_n33", "no_rescale") == (False, False)           # one tile per run: the mutation does not exist
    assert _fails("rp4_h24_hs2_n17", "merge_without_maxima")[0] and _fails("u_h24_hs2_n17", "merge_without_maxima")[0]
    assert _fails("rp4_h24_hs2_n17", "drop_last_run")[0] and _fails("u_h24_hs2_n17", "drop_last_run")[0]
    assert _fails("rp4_h16_hs4_n16", "drop_last_run") == (False, False)       # one run: nothing to drop
    assert _fails("rp4_h24_hs2_n17", "head_plus_one")[0] and _fails("u_h24_hs2_n17", "head_plus_one")[0]


def test_scale_restatement():
    for name, B, N, H, q_ld in fc.SCALE_CASES:
        q, gk, x = fc.scale_inputs(name)
        wv, qx = fr.scale_f32(q, gk, x)
        assert not fc.check_scale(name, wv, qx)[0]
        with np.errstate(all="ignore"):
            assert fc.check_scale(name, wv, (x + q * f32(1.0000001)).astype(f32))[0]         # a changed operand is seen
            assert fc.check_scale(name, (gk[:, None, :] * x).astype(f32), qx)[0]
        fin = np.isfinite(q) & np.isfinite(x)
        assert np.isinf(q).any() and (q == 0).any() and (np.abs(q[fin & (q != 0)]) < 1.2e-38).any()   # infinities, zeros, subnormals
    tot = {c[0]: c[1] * c[2] * c[3] for c in fc.SCALE_CASES}
    assert tot["total_4096"] % 1024 == 0 and tot["total_1032"] % 1024 != 0 and any(c[3] == 4 for c in fc.SCALE_CASES) and any(c[4] == 2 * c[3] for c in fc.SCALE_CASES)


# ---------------------------------------------------------------- refusals (no GPU needed)
def test_every_refusal_of_the_two_wrappers():
    import fastformer_harness as fh
    P = 0x10000                                                               # 'present', 16-byte aligned, never dereferenced

    def pool(v=P, v_ld=8, scale=None, wl=P, bl=P, lens=None, out=P, ws=P, ws_bytes=1 << 20, B=2, N=5, H=8, hs=2):
        return fh.ff_pool(v, v_ld, scale, wl, bl, lens, out, ws, ws_bytes, B, N, H, hs)

    for kw in (dict(v=None), dict(wl=None), dict(bl=None), dict(out=None), dict(ws=None)):
        assert pool(**kw) == "ff_pool: null pointer", kw
    for kw in (dict(B=0), dict(B=65536), dict(N=0), dict(N=(1 << 24) + 1)):
        assert pool(**kw) == "ff_pool: bad batch / sequence size", kw
    for kw in (dict(H=0), dict(H=6, v_ld=8), dict(H=1028, v_ld=1028)):
        assert pool(**kw) == "ff_pool: hidden must be a multiple of 4 in (0, 1024]", kw
    for hs in (0, 3, 16, -1):
        assert pool(hs=hs) == "ff_pool: head size must be 1, 2, 4 or 8"
    for kw in (dict(H=12, v_ld=12, hs=8), dict(H=1024, v_ld=1024, hs=1)):
        assert pool(**kw) == "ff_pool: hidden / head size must be an integer of at most 512", kw
    for v_ld in (4, 7, 10):
        assert pool(v_ld=v_ld) == "ff_pool: row stride must be a multiple of 4 and at least hidden"
    for kw in (dict(v=P + 4), dict(scale=P + 8), dict(out=P + 4), dict(ws=P + 12)):
        assert pool(**kw) == "ff_pool: unaligned pointer", kw
    need = fh.workspace_bytes(2, 5, 8, 2)
    assert need == 2 * 1 * 4 * 4 * 4 and pool(ws_bytes=need - 1) == "ff_pool: workspace too small" and pool(ws_bytes=0) == "ff_pool: workspace too small"

    def scale(q=P, q_ld=8, gk=P, x=P, wv=P, qx=P, B=2, N=5, H=8):
        return fh.ff_scale(q, q_ld, gk, x, wv, qx, B, N, H)

    for kw in (dict(q=None), dict(gk=None), dict(x=None), dict(wv=None), dict(qx=None)):
        assert scale(**kw) == "ff_scale: null pointer", kw
    for kw in (dict(B=0), dict(N=0), dict(H=0), dict(H=6), dict(q_ld=4), dict(q_ld=9), dict(B=-1)):
        assert scale(**kw) == "ff_scale: bad dims", kw
    for kw in (dict(q=P + 4), dict(gk=P + 8), dict(x=P + 4), dict(wv=P + 4), dict(qx=P + 12)):
        assert scale(**kw) == "ff_scale: unaligned pointer", kw
    assert scale(B=1 << 20, N=1 << 20, H=4, q_ld=4) == "ff_scale: too many elements"
