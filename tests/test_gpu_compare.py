"""The comparison library on the GPU (libe2etts_compare_test.so) against the float64 restatement (tests/compare_ref.py): the cepstra
element by element under a derived bar, the search's paths exactly -- on seeded features whose margins tests/golden/compare_cases.npz
records, on tie-rich 1-D and integer features, under bands, in sync mode --, every pair of a ragged batch against its own B = 1 call
bit for bit, and the figures.  Outputs are written into guarded buffers and the workspace is poisoned between calls."""
import ctypes as C

import numpy as np
import pytest

import compare_cases as cc
import compare_ref as cr
from e2e_tts_amd import compare as cmplib

pytestmark = pytest.mark.gpu

GUARD = 64
FIELDS_F = ("dist_total", "mcd_db", "mel_l1", "f0_rmse_hz", "f0_rmse_cents")
FIELDS_I = ("n_path", "n_voiced_both", "n_vuv_mismatch", "status")


@pytest.fixture(scope="module")
def cmp():
    c = cmplib.Comparator(20, 13, basis=np.random.default_rng(7).standard_normal((13, 20)).astype(np.float32))
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return cc.load()


def run_guarded(c, mode="dtw", band=None, hook=False):
    """``run`` through the raw entry points with guarded result and path buffers, after which the workspace is poisoned and the sides
    are gone: the next call sets them again.  -> list of dicts with "path"."""
    n = c._sides[0][0]
    buf = np.zeros(n + 2 * GUARD, cmplib.RESULT_DTYPE)
    raw = buf.view(np.uint8)
    raw[:] = 0xA5
    res = buf[GUARD:GUARD + n]
    fn = c.lib.e2ecmp_debug_run if hook else c.lib.e2ecmp_run
    c._check(fn(c._h, cmplib.DTW if mode == "dtw" else cmplib.SYNC, -1 if band is None else int(band), res.ctypes.data), "run")
    assert (buf[:GUARD].view(np.uint8) == 0xA5).all() and (buf[GUARD + n:].view(np.uint8) == 0xA5).all()
    out = []
    for b in range(n):
        d = {k: int(res[k][b]) for k in FIELDS_I}
        d.update({k: float(res[k][b]) for k in FIELDS_F})
        k = d["n_path"]
        pb = np.full(2 * (k + 2 * GUARD), -77, np.int32)
        got = C.c_longlong(-1)
        c._check(c.lib.e2ecmp_fetch_path(c._h, b, pb[2 * GUARD:].ctypes.data, k, C.byref(got)), "fetch_path")
        assert got.value == k and (pb[:2 * GUARD] == -77).all() and (pb[2 * GUARD + 2 * k:] == -77).all()
        d["path"] = pb[2 * GUARD:2 * GUARD + 2 * k].reshape(k, 2).copy()
        out.append(d)
    c.poison_workspace()
    return out


def set_pair(c, a, b):
    c.set_features("a", a[None], [len(a)])
    c.set_features("b", b[None], [len(b)])


def rel(x, y):
    return abs(x - y) / max(abs(y), 1e-300)


def check_against(got, want, tol=1e-12):
    """One pair's figures against the restatement's: integers and the path exactly, doubles to ``tol`` relative, NaN where it has NaN."""
    for k in FIELDS_I:
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["path"], want["path"])
    for k in FIELDS_F:
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (k, got[k])
        else:
            print(f"{k}: {got[k]!r} against {want[k]!r} (relative {rel(got[k], want[k]):.1e})")
            assert got[k] == want[k] or rel(got[k], want[k]) <= tol, (k, got[k], want[k])


# ---- cepstra
@pytest.mark.parametrize("n_mel", [80, 20])
@pytest.mark.parametrize("n_cep", [1, 13, 64])
def test_cepstra_against_float64(n_mel, n_cep):
    """T in {1, 15, 16, 17, 257} as one ragged batch (257 frames are five tiles of 64): every element under n_mel fp32 roundings times
    sum |terms|, rows past a length 0, and a row of the batch equal to its own B = 1 call bit for bit."""
    rng = np.random.default_rng([n_mel, n_cep])
    basis = rng.standard_normal((n_cep, n_mel)).astype(np.float32)
    lens = np.array([1, 15, 16, 17, 257])
    T = 257
    mel = (rng.standard_normal((len(lens), T, n_mel)) * 2.0 - 5.0).astype(np.float32)
    c = cmplib.Comparator(n_mel, n_cep, basis=basis)
    try:
        c.set_a(mel, lens)
        buf = np.full(GUARD + mel.shape[0] * T * n_cep + GUARD, 1234.5, np.float32)
        out = c.features("a", out=buf[GUARD:-GUARD]).reshape(len(lens), T, n_cep)
        assert (buf[:GUARD] == 1234.5).all() and (buf[-GUARD:] == 1234.5).all()
        worst = 0.0
        for b, n in enumerate(lens):
            want, bar = cr.cepstra(mel[b, :n], basis)
            err = np.abs(out[b, :n].astype(np.float64) - want)
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
            assert (err <= bar).all(), (b, float((err / bar).max()))
            assert not out[b, n:].any()
        print(f"n_mel {n_mel} n_cep {n_cep}: largest error / bar {worst:.3f}")
        c.poison_workspace()
        c.set_b(mel[3:4, :17], [17])
        assert np.array_equal(c.features("b")[0], out[3, :17])
    finally:
        c.close()


def test_cepstra_default_basis_and_odd_mel_count():
    """The default basis at (80, 13), and a mel count that is no multiple of 4 (the scalar staging path)."""
    rng = np.random.default_rng(3)
    for n_mel, n_cep, basis in ((80, 13, None), (18, 5, rng.standard_normal((5, 18)).astype(np.float32))):
        c = cmplib.Comparator(n_mel, n_cep, basis=basis)
        try:
            mel = (rng.standard_normal((2, 70, n_mel)) - 4.0).astype(np.float32)
            c.set_a(mel, [70, 33])
            out = c.features("a")
            for b, n in enumerate((70, 33)):
                want, bar = cr.cepstra(mel[b, :n], c.basis)
                assert (np.abs(out[b, :n] - want) <= bar).all()
        finally:
            c.close()


# ---- the search
@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("Ta,Tb", cc.PAIRS)
def test_search_on_given_features(cmp, golden, Ta, Tb, D):
    """The path equals the restatement's exactly and dist_total to 1e-12 relative.  D >= 2: seeds whose smallest margin on the path is at
    least 1e-9 of dist_total (recorded; no decision is left out).  D = 1: costs exact in double, exact ties on the path, no filter: a
    wrong tie order or a square root that is not correctly rounded shows here."""
    g = golden[f"s{Ta}x{Tb}x{D}"]
    a, b = cc.features(Ta, Tb, D, g["seed"])
    want, s = cr.compare(a, b)
    assert want["n_path"] == g["n_path"] and rel(want["dist_total"], g["dist_total"]) <= 1e-12   # the inputs are the recorded ones
    if D >= 2:
        assert s["path_margin"] >= cc.MIN_MARGIN * s["dist_total"]
    set_pair(cmp, a, b)
    got = run_guarded(cmp)[0]
    check_against(got, want)
    assert got["dist_total"] == want["dist_total"]   # the same operations in the same order: not one bit apart


def test_ties_are_exact_on_the_tie_rich_cases(golden):
    """What the 1-D cases are for: the recorded path of (40, 300) and its like holds decisions with margin exactly 0."""
    assert golden["s40x300x1"]["path_margin"] == 0.0 and golden["s255x257x1"]["path_margin"] == 0.0


def test_ragged_batch_equals_single_calls(cmp, golden):
    """B = 3 with lens (257, 64, 1) against (5, 300, 1): each pair equals its own B = 1 call bit for bit, and the restatement."""
    D = cc.RAGGED_D
    pairs = [cc.features(Ta, Tb, D, golden[f"r{Ta}x{Tb}x{D}"]["seed"]) for Ta, Tb in zip(cc.RAGGED_A, cc.RAGGED_B)]
    fa, fb = np.zeros((3, max(cc.RAGGED_A), D), np.float32), np.zeros((3, max(cc.RAGGED_B), D), np.float32)
    for k, (a, b) in enumerate(pairs):
        fa[k, :len(a)], fb[k, :len(b)] = a, b
    fa[1, 64:], fb[0, 5:] = 9e9, -9e9   # what lies past a length is not read
    cmp.set_features("a", fa, cc.RAGGED_A)
    cmp.set_features("b", fb, cc.RAGGED_B)
    batch = run_guarded(cmp)
    for k, (a, b) in enumerate(pairs):
        set_pair(cmp, a, b)
        one = run_guarded(cmp)[0]
        for f in FIELDS_I:
            assert batch[k][f] == one[f]
        for f in FIELDS_F:
            assert np.float64(batch[k][f]).tobytes() == np.float64(one[f]).tobytes(), f
        assert np.array_equal(batch[k]["path"], one["path"])
        check_against(one, cr.compare(a, b)[0])


def test_integer_features_with_engineered_ties(cmp):
    """Constant sequences: every decision is a three-way tie, the path is the diagonal from the end until an index reaches 0, then
    straight.  Multiples of (3, 4): every cost is 5 |n - m|, an integer, and ties abound; D = 3 small integers: costs are square roots
    of small integers, equal wherever the integers are."""
    for Ta, Tb in ((9, 4), (4, 9), (6, 6), (300, 70)):
        a, b = np.full((Ta, 2), 3.0, np.float32), np.full((Tb, 2), 3.0, np.float32)
        set_pair(cmp, a, b)
        got = run_guarded(cmp)[0]
        n = max(Ta, Tb)
        i = np.maximum(np.arange(n) - (n - Ta), 0)
        j = np.maximum(np.arange(n) - (n - Tb), 0)
        assert np.array_equal(got["path"], np.stack([i, j], 1)) and got["dist_total"] == 0.0 and got["mcd_db"] == 0.0
        check_against(got, cr.compare(a, b)[0])
    rng = np.random.default_rng(11)
    for Ta, Tb in ((70, 300), (257, 130)):
        n, m = rng.integers(0, 4, Ta), rng.integers(0, 4, Tb)
        a, b = (n[:, None] * np.array([3.0, 4.0])).astype(np.float32), (m[:, None] * np.array([3.0, 4.0])).astype(np.float32)
        want, s = cr.compare(a, b)
        assert (s["margin"][want["path"][1:, 0], want["path"][1:, 1]] == 0).any()   # exact ties on the path
        set_pair(cmp, a, b)
        check_against(run_guarded(cmp)[0], want)
        a, b = rng.integers(0, 3, (Ta, 3)).astype(np.float32), rng.integers(0, 3, (Tb, 3)).astype(np.float32)
        set_pair(cmp, a, b)
        check_against(run_guarded(cmp)[0], cr.compare(a, b)[0])


def test_more_shapes_three_chunks_the_widest_rows_and_the_cap(cmp):
    """Shapes beyond the listed ones, judged by the restatement alone: three chunks of thread rows (S = 640), D = 64 (the widest register
    row), D = 4 and 5 (a whole 16-byte word, and one more), and the frame cap: 4096 frames against 300 (the longest row a chunk hands on,
    the largest index a path cell packs)."""
    for Ta, Tb, D in ((700, 640, 4), (65, 63, 64), (130, 257, 5), (4096, 300, 2)):
        a, b = cc.features(Ta, Tb, D, 0)
        want, s = cr.compare(a, b)
        assert s["path_margin"] >= cc.MIN_MARGIN * s["dist_total"]
        set_pair(cmp, a, b)
        check_against(run_guarded(cmp)[0], want)


@pytest.mark.parametrize("band", cc.BANDS)
@pytest.mark.parametrize("Ta,Tb", cc.BAND_PAIRS)
def test_band(cmp, golden, Ta, Tb, band):
    g = golden[f"b{band}_{Ta}x{Tb}x13"]
    a, b = cc.features(Ta, Tb, 13, g["seed"])
    want, s = cr.compare(a, b, band=band)
    assert want["status"] == 0 and s["path_margin"] >= cc.MIN_MARGIN * s["dist_total"]
    allowed = cr.band_mask(Ta, Tb, band)
    assert allowed[want["path"][:, 0], want["path"][:, 1]].all()
    set_pair(cmp, a, b)
    check_against(run_guarded(cmp, band=band)[0], want)


def test_pairs_without_a_path_leave_the_others_alone(cmp):
    """Every band >= 1 holds a path (tests/test_compare_host.py enumerates it), so the pairs without one are made with the two means
    there are: band 0 through the test hook -- only cells exactly on the line i * Tb == j * Ta, which (7, 1) and (63, 64) cannot walk and
    (6, 6) can --, and an infinite frame under band 1, 2 and 8 through the public entry.  Such a pair gets status 1 and NaN figures; its
    neighbours in the batch equal the restatement."""
    shapes = ((6, 6), (7, 1), (63, 64), (2, 2))
    pairs = [cc.features(Ta, Tb, 13, 5) for Ta, Tb in shapes]
    fa, fb = np.zeros((4, 63, 13), np.float32), np.zeros((4, 64, 13), np.float32)
    for k, (a, b) in enumerate(pairs):
        fa[k, :len(a)], fb[k, :len(b)] = a, b

    def both():
        cmp.set_features("a", fa, [s[0] for s in shapes])
        cmp.set_features("b", fb, [s[1] for s in shapes])

    both()
    with pytest.raises(ValueError, match="band must be at least 1"):
        cmp.run(band=0)
    got = run_guarded(cmp, band=0, hook=True)
    assert [g["status"] for g in got] == [0, 1, 1, 0]
    for k, (a, b) in enumerate(pairs):
        check_against(got[k], cr.compare(a, b, band=0)[0])
    fa[2, 31] = np.inf   # every path of pair 2 crosses row 31
    for band in cc.BANDS:
        both()
        got = run_guarded(cmp, band=band)
        assert [g["status"] for g in got] == [0, 0, 1, 0]
        assert got[2]["n_path"] == 0 and all(np.isnan(got[2][f]) for f in FIELDS_F)
        for k in (0, 1, 3):
            check_against(got[k], cr.compare(*pairs[k], band=band)[0])


def test_sync_mode(cmp):
    for Ta, Tb, D in ((1, 1, 13), (300, 257, 13), (64, 300, 1), (257, 257, 32)):
        a, b = cc.features(Ta, Tb, D, 2)
        set_pair(cmp, a, b)
        got = run_guarded(cmp, mode="sync")[0]
        want = cr.compare(a, b, mode="sync")[0]
        assert got["n_path"] == min(Ta, Tb) and np.array_equal(got["path"][:, 0], got["path"][:, 1])
        check_against(got, want)


# ---- the figures
def tracks(rng, T, kind):
    """An f0 track with voiced and unvoiced runs."""
    f = rng.uniform(90.0, 400.0, T)
    runs = np.repeat(rng.random(T // 7 + 1) > 0.4, 7)[:T]
    if kind == "voiced":
        runs[:] = True
    if kind == "unvoiced":
        runs[:] = False
    return np.where(runs, f, 0.0).astype(np.float32)


@pytest.mark.parametrize("kind", ["runs", "no_f0", "never_both", "one_side_f0"])
@pytest.mark.parametrize("mode", ["dtw", "sync"])
def test_figures(cmp, mode, kind):
    """From mels: the restatement runs on the cepstra the library made (fetched), so the search is compared on equal inputs, and takes
    mel L1 and the f0 figures from the same mels and tracks.  1e-12 relative."""
    rng = np.random.default_rng(17)
    la, lb = np.array([257, 40, 90]), np.array([230, 64, 90])
    ma = (rng.standard_normal((3, 257, 20)) - 4.0).astype(np.float32)
    mb = np.zeros((3, 230, 20), np.float32)
    for k in range(3):
        src = np.linspace(0, la[k] - 1, lb[k]).round().astype(int)
        mb[k, :lb[k]] = ma[k, src] + 0.2 * rng.standard_normal((lb[k], 20))
    fa = np.stack([tracks(rng, 257, "runs") for _ in range(3)])
    fb = np.stack([tracks(rng, 230, "runs") for _ in range(3)])
    if kind == "never_both":
        fa[:] = 0.0
    if kind == "no_f0":
        fa = fb = None
    cmp.set_a(ma, la, fa)
    cmp.set_b(mb, lb, None if kind == "one_side_f0" else fb)
    ca, cb = cmp.features("a"), cmp.features("b")
    got = run_guarded(cmp, mode=mode)
    use_f0 = kind in ("runs", "never_both")
    for k in range(3):
        want = cr.compare(ca[k, :la[k]], cb[k, :lb[k]], mode=mode, mel_a=ma[k], mel_b=mb[k], f0_a=fa[k] if use_f0 else None, f0_b=fb[k] if use_f0 else None)[0]
        check_against(got[k], want)
        if kind == "runs":
            assert got[k]["n_voiced_both"] > 0 and got[k]["n_vuv_mismatch"] > 0 and got[k]["f0_rmse_hz"] > 0
        if kind == "never_both":
            assert got[k]["n_voiced_both"] == 0 and got[k]["n_vuv_mismatch"] > 0 and np.isnan(got[k]["f0_rmse_hz"]) and np.isnan(got[k]["f0_rmse_cents"])
        if not use_f0:
            assert got[k]["n_voiced_both"] == 0 and got[k]["n_vuv_mismatch"] == 0 and np.isnan(got[k]["f0_rmse_hz"])
        assert got[k]["mel_l1"] > 0


def test_a_side_stays_resident_and_features_give_no_mel_l1(cmp):
    """Side A set once, side B set twice: the second run equals a fresh handle's; a side set from features has no mel L1."""
    rng = np.random.default_rng(23)
    ma = (rng.standard_normal((1, 50, 20)) - 4.0).astype(np.float32)
    mb1, mb2 = ma[:, ::-1].copy(), (ma + 0.1).astype(np.float32)
    cmp.set_a(ma, [50])
    cmp.set_b(mb1, [50])
    cmp.run()
    cmp.set_b(mb2, [50])
    second = cmp.run(return_path=True)[0]
    cmp.poison_workspace()
    cmp.set_a(ma, [50])
    cmp.set_b(mb2, [50])
    fresh = cmp.run(return_path=True)[0]
    assert all(np.array_equal(np.asarray(second[k]), np.asarray(fresh[k]), equal_nan=True) for k in second)
    cb = cmp.features("b")
    cmp.set_features("b", cb, [50])
    mixed = cmp.run()[0]
    assert np.isnan(mixed["mel_l1"]) and mixed["dist_total"] == fresh["dist_total"]
    with pytest.raises(ValueError, match="the sides differ"):
        cmp.set_features("b", cb[:, :, :5].copy(), [50])
        cmp.run()
    cmp.poison_workspace()
    with pytest.raises(RuntimeError, match="both sides"):
        cmp.run()
