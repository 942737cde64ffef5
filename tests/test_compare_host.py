"""The comparison library, the parts that need no GPU: the float64 restatement (tests/compare_ref.py) against brute force and on
constructed ties, the band predicate of csrc/compare/plan.h, the default basis, the committed seeds under the filter the GPU tests rely
on, and the companion library's C ABI -- its exports and the refusals that come before a device is opened."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import compare_cases as cc
import compare_ref as cr
from e2e_tts_amd import compare as cmplib


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_compare_hash() != g.compare_hash() or g.built_compare_hash(g.COMPARE["test_lib"]) != g.compare_hash():
        g.build()
    return cmplib.load_library()


def test_dp_minimum_equals_brute_force():
    """Every Ta, Tb <= 5, continuous and tie-rich integer costs: the recurrence's total is the smallest over all monotone paths, and the
    path it returns is monotone, runs from (0, 0) to the end and sums to that total."""
    rng = np.random.default_rng(0)
    for Ta, Tb in itertools.product(range(1, 6), repeat=2):
        for kind in ("gauss", "int"):
            if kind == "gauss":
                a, b = rng.standard_normal((Ta, 3)).astype(np.float32), rng.standard_normal((Tb, 3)).astype(np.float32)
            else:
                a, b = rng.integers(0, 3, (Ta, 1)).astype(np.float32), rng.integers(0, 3, (Tb, 1)).astype(np.float32)
            d = cr.cost_matrix(a, b)
            s = cr.search(d)
            bf = cr.brute_force(d)
            assert s["status"] == 0 and (s["dist_total"] == bf if kind == "int" else abs(s["dist_total"] - bf) <= 1e-12 * max(bf, 1.0))
            p = s["path"]
            assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (Ta - 1, Tb - 1)
            steps = np.diff(p, axis=0)
            assert all(tuple(st) in ((1, 1), (1, 0), (0, 1)) for st in steps)
            assert abs(d[p[:, 0], p[:, 1]].sum() - s["dist_total"]) <= 1e-12 * max(bf, 1.0)


def test_cost_is_the_explicit_loop():
    """k ascending, product and sum as separate roundings: against a scalar loop, bit for bit."""
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((4, 13)).astype(np.float32), rng.standard_normal((3, 13)).astype(np.float32)
    d = cr.cost_matrix(a, b)
    for i in range(4):
        for j in range(3):
            acc = np.float64(0.0)
            for k in range(13):
                diff = np.float64(a[i, k]) - np.float64(b[j, k])
                acc = acc + diff * diff
            assert d[i, j] == np.sqrt(acc)


def test_tie_order_on_constant_sequences():
    """All costs 0: every decision is a three-way tie.  Diagonal first, then (i-1, j), then (i, j-1): from the end the path is the
    diagonal until an index reaches 0, then straight."""
    for Ta, Tb in ((9, 4), (4, 9), (6, 6), (1, 5), (5, 1)):
        s = cr.search(cr.cost_matrix(np.ones((Ta, 2), np.float32), np.ones((Tb, 2), np.float32)))
        n = max(Ta, Tb)
        want = np.stack([np.maximum(np.arange(n) - (n - Ta), 0), np.maximum(np.arange(n) - (n - Tb), 0)], 1)
        assert np.array_equal(s["path"], want) and s["dist_total"] == 0.0
        if min(Ta, Tb) > 1:
            assert s["path_margin"] == 0.0
    # two-way ties: (i-1, j) before (i, j-1)
    d = np.array([[0.0, 1.0], [1.0, 5.0]])
    s = cr.search(d)
    assert s["code"][1, 1] == 0 and np.array_equal(s["path"], [[0, 0], [1, 1]])
    d = np.zeros((3, 3))
    d[1, 1] = 100.0   # at (2, 2): (1, 2) and (2, 1) tie at 0 below the diagonal's 100; at (1, 2): the diagonal and (0, 2) tie
    s = cr.search(d)
    assert s["code"][2, 2] == 1 and s["margin"][2, 2] == 0.0 and s["code"][1, 2] == 0 and s["code"][2, 1] == 0
    assert np.array_equal(s["path"], [[0, 0], [0, 1], [1, 2], [2, 2]])


def test_band_predicate():
    """Symmetric in the two sequences; both end cells allowed for every band >= 1; every band >= 1 holds a path (the cells nearest the
    line i / Ta = j / Tb are connected), so only the narrowest band, 0 -- cells exactly on the line --, gives none; no band allows all."""
    for Ta, Tb in itertools.product((1, 2, 3, 5, 7, 12, 40, 63, 64), repeat=2):
        for band in (0, 1, 2, 8):
            m = cr.band_mask(Ta, Tb, band)
            assert np.array_equal(m, cr.band_mask(Tb, Ta, band).T)
            assert m[0, 0]
            if band >= 1:
                assert m[-1, -1]
                assert cr.search(np.ones((Ta, Tb)), band)["status"] == 0
        assert cr.band_mask(Ta, Tb, -1).all()
        i, j = np.arange(Ta)[:, None], np.arange(Tb)[None, :]
        assert np.array_equal(cr.band_mask(Ta, Tb, 2), np.abs(i * Tb - j * Ta) <= 2 * max(Ta, Tb))
    assert cr.search(np.ones((7, 1)), 0)["status"] == 1 and cr.search(np.ones((63, 64)), 0)["status"] == 1
    assert cr.search(np.ones((6, 6)), 0)["status"] == 0 and len(cr.search(np.ones((6, 6)), 0)["path"]) == 6
    assert cr.shim().e2ecmp_shim_max_t() == cmplib.MAX_T
    # a band narrows the search: the banded total is never below the free one
    a, b = cc.features(63, 64, 13, 0)
    d = cr.cost_matrix(a, b)
    assert cr.search(d, 1)["dist_total"] >= cr.search(d, 8)["dist_total"] >= cr.search(d)["dist_total"]


def test_default_basis_is_orthonormal_without_row_0():
    for n_mel, n_cep in ((80, 13), (20, 13), (80, 64)):
        bs = cmplib.default_basis(n_mel, n_cep)
        assert bs.shape == (n_cep, n_mel) and bs.dtype == np.float32
        full = cmplib.dct_matrix(n_mel)
        assert np.abs(full @ full.T - np.eye(n_mel)).max() <= 1e-13
        assert np.abs(bs.astype(np.float64) @ bs.astype(np.float64).T - np.eye(n_cep)).max() <= 4 * n_mel * 2.0 ** -24
        assert np.abs(bs - full[1:n_cep + 1]).max() <= 2.0 ** -24 and np.abs(bs - cr.dct_basis(n_mel, n_cep)).max() <= 2.0 ** -24
        assert np.abs(bs.astype(np.float64).sum(1)).max() <= n_mel * 2.0 ** -24      # no row is c0: a constant frame has zero cepstra
    try:
        from scipy.fft import dct
    except ImportError:
        dct = None
    if dct is not None:
        x = np.random.default_rng(2).standard_normal(80)
        assert np.abs(cmplib.dct_matrix(80) @ x - dct(x, type=2, norm="ortho")).max() <= 1e-12
        assert np.abs(cmplib.dct_matrix(80) - dct(np.eye(80), type=2, norm="ortho", axis=0)).max() <= 1e-13
    with pytest.raises(ValueError, match="n_cep in"):
        cmplib.default_basis(13, 13)


def test_identical_inputs_have_mcd_exactly_0():
    rng = np.random.default_rng(3)
    for T, D in ((1, 13), (37, 13), (64, 1)):
        a = rng.standard_normal((T, D)).astype(np.float32)
        for mode in ("dtw", "sync"):
            r = cr.compare(a, a.copy(), mode=mode, f0_a=np.full(T, 200.0, np.float32), f0_b=np.full(T, 200.0, np.float32))[0]
            assert r["mcd_db"] == 0.0 and r["dist_total"] == 0.0 and r["f0_rmse_hz"] == 0.0 and r["f0_rmse_cents"] == 0.0
            assert np.array_equal(r["path"][:, 0], r["path"][:, 1]) and r["n_path"] == T and r["n_voiced_both"] == T


def test_figures_on_a_hand_made_path():
    d = np.array([[3.0, 9.0], [9.0, 1.0]])
    r = cr.figures(np.array([[0, 0], [1, 1]]), d, np.array([[1.0, 2.0], [3.0, 4.0]], np.float32), np.array([[1.0, 4.0], [0.0, 4.0]], np.float32),
                   np.array([100.0, 0.0], np.float32), np.array([200.0, 50.0], np.float32))
    assert r["mcd_db"] == cr.MCD_SCALE * 2.0 and r["mel_l1"] == (0 + 2 + 3 + 0) / 4 and r["n_voiced_both"] == 1 and r["n_vuv_mismatch"] == 1
    assert r["f0_rmse_hz"] == 100.0 and r["f0_rmse_cents"] == 1200.0
    assert abs(cr.MCD_SCALE - 6.141851463713754) < 1e-12 and cmplib.MCD_SCALE == cr.MCD_SCALE


def test_committed_seeds_pass_the_filter():
    """With the restatement alone: every recorded case is reproduced from its seed, is the first seed that passes, and -- for D >= 2 --
    keeps its smallest margin on the path at 1e-9 of dist_total or more.  The 1-D cases hold exact ties on their paths."""
    g = cc.load()
    cases = cc.case_list()
    assert sorted(g) == sorted(c[0] for c in cases)
    for name, Ta, Tb, D, band in cases:
        seed, s = cc.first_good_seed(Ta, Tb, D, band)
        r = g[name]
        assert seed == r["seed"] and len(s["path"]) == r["n_path"]
        assert s["dist_total"] == r["dist_total"] and (s["path_margin"] == r["path_margin"])
        if D >= 2:
            assert s["path_margin"] >= cc.MIN_MARGIN * s["dist_total"]
    assert g["s40x300x1"]["path_margin"] == 0.0 and g["s255x257x1"]["path_margin"] == 0.0 and g["s513x511x1"]["path_margin"] == 0.0


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_compare.h")).read()
    hooks_block = re.search(r"#ifdef E2ECMP_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2ecmp_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2ECMP_API [^;]*?\b(e2ecmp_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(cmplib.TEST_HOOK_SYMBOLS) and declared == sorted(cmplib.EXPORTED_SYMBOLS)
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "compare", "compare.map")).read()
    assert re.search(r"global:\s*e2ecmp_\*;\s*local:\s*\*;", vmap)
    # the export count, as the header, the version script and the README state it
    n, k = len(declared), len(hook_syms)
    assert f"Exports: {n} entry points, and {k} more in the test build" in header and f"({n}, and {k} more in the test build)" in vmap
    assert f"{n} exports" in open(os.path.join(ROOT, "README.md")).read()

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(cmplib.LIB_PATH) == declared, sorted(set(exported(cmplib.LIB_PATH)) ^ set(declared))     # the product library: no test hook
    assert exported(cmplib.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(cmplib.LIB_PATH)                                                                        # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2ecmp_abi_version() == cmplib.ABI_VERSION == int(re.search(r"#define E2ECMP_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2ECMP_MAX_B", cmplib.MAX_B), ("E2ECMP_MAX_T", cmplib.MAX_T), ("E2ECMP_MAX_D", cmplib.MAX_D), ("E2ECMP_MAX_MEL", cmplib.MAX_MEL),
                      ("E2ECMP_A", cmplib.A), ("E2ECMP_B", cmplib.B), ("E2ECMP_DTW", cmplib.DTW), ("E2ECMP_SYNC", cmplib.SYNC)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    assert C.sizeof(cmplib.CResult) == 72 == cmplib.RESULT_DTYPE.itemsize
    assert [f[0] for f in cmplib.CResult._fields_] == list(cmplib.RESULT_DTYPE.names)
    import __graft_entry__ as g
    assert g.compare_hash() in lib.e2ecmp_version().decode()
    assert any(os.path.basename(f) == "plan.h" for f in g.COMPARE["extra"]) and g.COMPARE in g.COMPANIONS
    # the other libraries are untouched: nothing of the companion is exported there
    from e2e_tts_amd import _lib, aligner as al, mel as mp, resample as rsl, condition as cdl, f0 as f0l
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH, al.LIB_PATH, mp.LIB_PATH, rsl.LIB_PATH, cdl.LIB_PATH, f0l.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2ecmp_" not in syms
    for f in ("compare.hip", "plan.h"):
        assert "getenv" not in open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "compare", f)).read()
    assert "hip" not in open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "compare", "plan.h")).read().lower().replace("__hipcc__", "").replace("hip-free", "").replace("compare.hip", "")


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and nothing was allocated."""
    P = C.c_void_p
    h = P()
    assert lib.e2ecmp_create(0, 80, 13, None) == cmplib.E_INVAL and lib.e2ecmp_create(-1, 80, 13, C.byref(h)) == cmplib.E_INVAL and not h.value
    for n_mel, n_cep, word in ((0, 13, b"n_mel"), (1025, 13, b"n_mel"), (80, 0, b"n_cep"), (80, 65, b"n_cep"), (1024, 64, b"LDS")):
        assert lib.e2ecmp_create(0, n_mel, n_cep, C.byref(h)) == cmplib.E_INVAL and word in lib.e2ecmp_last_error(None) and not h.value
    assert lib.e2ecmp_create(0, 80, 13, C.byref(h)) == cmplib.E_OK and h.value
    assert lib.e2ecmp_load(h, None) == cmplib.E_INVAL
    bad = cmplib.default_basis(80, 13).copy()
    bad[3, 5] = np.nan
    assert lib.e2ecmp_load(h, bad.ctypes.data) == cmplib.E_INVAL and b"finite" in lib.e2ecmp_last_error(h)
    mel, f0, x = np.zeros((2, 9, 80), np.float32), np.zeros((2, 9), np.float32), np.zeros((2, 9, 13), np.float32)
    lens = np.array([9, 4], np.int64)
    sm = lambda side, m, ln, B, T: lib.e2ecmp_set_mels(h, side, None if m is None else m.ctypes.data, f0.ctypes.data, None if ln is None else ln.ctypes.data, B, T)   # noqa: E731
    sf = lambda side, v, ln, B, T, D: lib.e2ecmp_set_features(h, side, None if v is None else v.ctypes.data, None if ln is None else ln.ctypes.data, B, T, D)   # noqa: E731
    assert sm(0, mel, lens, 2, 9) == cmplib.E_STATE and b"e2ecmp_load" in lib.e2ecmp_last_error(h)
    assert sm(2, mel, lens, 2, 9) == cmplib.E_INVAL and sm(0, None, lens, 2, 9) == cmplib.E_INVAL and sm(0, mel, None, 2, 9) == cmplib.E_INVAL
    assert sm(0, mel, lens, 0, 9) == cmplib.E_INVAL and sm(0, mel, lens, 4097, 9) == cmplib.E_INVAL and sm(0, mel, lens, 2, 4097) == cmplib.E_INVAL
    assert sf(0, None, lens, 2, 9, 13) == cmplib.E_INVAL and sf(0, x, lens, 2, 9, 0) == cmplib.E_INVAL and sf(0, x, lens, 2, 9, 65) == cmplib.E_INVAL
    assert sf(3, x, lens, 2, 9, 13) == cmplib.E_INVAL and sf(0, x, lens, 2, 0, 13) == cmplib.E_INVAL
    for ln in ([0, 4], [9, 10], [-1, 9]):
        assert sf(0, x, np.array(ln, np.int64), 2, 9, 13) == cmplib.E_INVAL and b"lens[" in lib.e2ecmp_last_error(h)
    res = np.zeros(2, cmplib.RESULT_DTYPE)
    assert lib.e2ecmp_run(h, 0, -1, res.ctypes.data) == cmplib.E_STATE and b"both sides" in lib.e2ecmp_last_error(h)
    assert lib.e2ecmp_run(h, 2, -1, res.ctypes.data) == cmplib.E_INVAL and lib.e2ecmp_run(h, 0, 0, res.ctypes.data) == cmplib.E_INVAL
    assert b"band" in lib.e2ecmp_last_error(h) and lib.e2ecmp_run(h, 0, 2 ** 41, res.ctypes.data) == cmplib.E_INVAL
    n = C.c_longlong(-5)
    assert lib.e2ecmp_fetch_path(h, 0, None, 0, C.byref(n)) == cmplib.E_STATE and n.value == -5
    assert lib.e2ecmp_fetch_features(h, 0, x.ctypes.data) == cmplib.E_STATE and lib.e2ecmp_fetch_features(h, 5, x.ctypes.data) == cmplib.E_INVAL
    assert lib.e2ecmp_device_bytes(h) == 0 and not res.view(np.uint8).any()
    ms = (C.c_double * 3)()
    assert lib.e2ecmp_profile_enable(h, 1) == cmplib.E_OK and lib.e2ecmp_profile_read(h, ms) == cmplib.E_OK and list(ms) == [0.0, 0.0, 0.0]
    assert lib.e2ecmp_profile_read(h, None) == cmplib.E_INVAL and lib.e2ecmp_sync(h) == cmplib.E_OK
    lib.e2ecmp_destroy(h)
    lib.e2ecmp_destroy(None)
    for fn in (lib.e2ecmp_sync, lib.e2ecmp_stream):
        assert not fn(None) or fn(None) == cmplib.E_INVAL
    with pytest.raises(ValueError, match="basis of shape"):
        cmplib.Comparator(80, 13, basis=np.zeros((12, 80), np.float32))
    with pytest.raises(ValueError, match="n_mel"):
        cmplib.Comparator(2000, 13, basis=np.zeros((13, 2000), np.float32))
