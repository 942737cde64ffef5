"""The corpus-statistics library, the parts that need no GPU: the numpy restatement (tests/stats_ref.py) against what the reference's own
text computed (tests/golden/stats_cases.npz, tools/make_stats_goldens.py) -- percentiles, fences and kept counts exactly, build_stats'
dict within the derived bars --, the bars against listed mutations, and the companion library's C ABI: its exports, its build-table
entry and the refusals that come before a device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import stats_cases as sc
import stats_ref as sr
from e2e_tts_amd import stats as stlib


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_stats_hash() != g.stats_hash() or g.built_stats_hash(g.STATS["test_lib"]) != g.stats_hash():
        g.build()
    return stlib.load_library()


@pytest.fixture(scope="module")
def gold():
    return sc.load()


@pytest.fixture(scope="module")
def corpora(gold):
    c = sc.corpora()
    for name, utts in c.items():
        assert np.array_equal(sc.digest(utts), gold[f"{name}/digest"]), f"the generator of corpus {name} drifted from the fixture"
    return c


def want_stats(gold, name):
    v = dict(zip(sc.STAT_KEYS, gold[f"{name}/stats"]))
    return {k: {f: float(v[f"{k}.{f}"]) for f in (("mean", "std") if k == "f0" else ("max", "min", "mean", "std"))} for k in ("f0", "pitch", "energy")}


def row_mismatches(gold, corpora, mut=None):
    """(corpus, kind, row, field) of every per-row figure that differs from the reference's, bit for bit."""
    bad = []
    for name, utts in corpora.items():
        for kind in ("energy", "pitch"):
            for i, u in enumerate(utts):
                r = sr.row_record(u[kind], sr.ENERGY, mut)
                for f in ("p25", "p75", "lower", "upper"):
                    if np.float32(r[f]).tobytes() != gold[f"{name}/{kind}/{f}"][i].tobytes():
                        bad.append((name, kind, i, f))
                if r["n_kept"] != gold[f"{name}/{kind}/kept"][i]:
                    bad.append((name, kind, i, "kept"))
    return bad


def test_cases_cover_what_the_issue_lists(corpora):
    lens = {len(u["energy"]) for utts in corpora.values() for u in utts}
    assert set(sc.LENGTHS) <= lens and sc.CAP == stlib.MAX_ROW
    assert all(len(corpora[f"ragged{i}"]) == 7 for i in range(3)) and len(corpora["twelve"]) == 12
    n_fence = 0
    for u in corpora["fences"]:
        _, _, lower, upper = sc.fences_of(u["energy"])
        n_fence += bool((u["energy"] == lower).any() or (u["energy"] == upper).any())
    assert n_fence >= 4
    f0 = [u["f0"] for u in corpora["voicing"]]
    assert any((x == 0).all() for x in f0) and any((x != 0).all() for x in f0) and any(np.signbit(x[x == 0]).any() for x in f0)


def test_virtual_indices_are_numpys():
    """lo, hi and gamma of the header against numpy's own virtual index arithmetic, and the percentile against np.percentile itself on
    random float32 rows of 1 to 300 values."""
    rng = np.random.default_rng(5)
    for n in list(range(1, 70)) + [127, 128, 129, 1000, 16384]:
        for q in (25, 75):
            v = (n - 1) * np.true_divide(q, 100)
            lo, hi, g = sr.vindex(n, q)
            assert lo == int(np.floor(v)) and hi == min(lo + 1, n - 1) and g == np.float32(v - np.floor(v))
    for _ in range(300):
        row = (rng.standard_normal(int(rng.integers(1, 301))) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
        _, p25, p75, lower, upper = sr.fences(row)
        want = sc.fences_of(row)
        assert all(np.float32(a).tobytes() == np.float32(b).tobytes() and np.asarray(b).dtype == np.float32 for a, b in zip((p25, p75, lower, upper), want))


def test_restatement_reproduces_the_reference_rows_exactly(gold, corpora):
    assert row_mismatches(gold, corpora) == []


def test_restatement_reproduces_build_stats_within_the_bars(gold, corpora):
    for name, utts in corpora.items():
        got, want = sr.corpus(utts), want_stats(gold, name)
        for k in ("f0", "energy", "pitch"):
            assert sr.check_block(got[k], want[k], got["_bars"][k], k != "f0") == [], (name, k)
    c = sr.corpus(corpora["constant"])
    assert c["energy"]["std"] == 1.0 and c["energy"]["mean"] == 5.0 and c["pitch"]["std"] == 1.0    # zero variance: sklearn's scale of a constant
    assert sr.row_record(corpora["constant"][1]["energy"])["n_kept"] == 0 and sr.row_record(corpora["constant"][2]["energy"])["n_kept"] == 0


def test_get_prosody_is_float32_arithmetic(gold, corpora):
    for name in ("ragged0", "ragged1", "ties", "fences", "constant"):
        st = want_stats(gold, name)["energy"]
        x, lens = sc.batch(corpora[name], "energy")
        got = sr.normalize(x, lens, st["mean"], st["std"])
        flat = np.concatenate([got[b, :n] for b, n in enumerate(lens)])
        assert flat.tobytes() == gold[f"{name}/energy/target"].tobytes()
        assert all((got[b, n:] == 0).all() for b, n in enumerate(lens))


def test_the_checks_fail_the_listed_mutations(gold, corpora):
    """What is exact catches a non-strict fence (on the rows where a value equals one) and the fused lerp (on the rows where it changes
    a bit); the bars catch one kept value dropped and the sample std."""
    closed = row_mismatches(gold, corpora, "closed_fences")
    assert {m[0] for m in closed} >= {"fences", "constant"} and {m[3] for m in closed} == {"kept"}
    assert sum(1 for m in closed if m[0] == "fences" and m[1] == "energy") >= 4
    fused = row_mismatches(gold, corpora, "fma_lerp")
    assert len(fused) >= 10 and {m[3] for m in fused} <= {"lower", "upper", "kept"}    # the lerp's product is exact at q = 25, 75: the fences show it
    for mut in ("drop_one", "sample_std"):
        for name in ("lengths", "ragged0", "twelve", "ties"):
            got, want = sr.corpus(corpora[name], mut), want_stats(gold, name)
            for k in ("f0", "energy", "pitch"):
                if mut == "drop_one" and k == "f0":
                    continue   # the mutation drops a value inside the fences
                assert sr.check_block(got[k], want[k], got["_bars"][k], k != "f0") != [], (mut, name, k)


def test_merge_does_not_depend_on_the_batching(corpora):
    """The restatement's fold is sequential by construction; here: the merged figures are the two-pass figures over all kept values
    within the bars (Chan's update is the same quantity)."""
    got = sr.corpus(corpora["twelve"])
    for k, kind in (("energy", sr.ENERGY), ("f0", sr.F0)):
        kept = np.concatenate([np.asarray(sr.row_record(u[k], kind)["kept"], np.float64) for u in corpora["twelve"]])
        N, sum_abs, total = got["_bars"][k]
        assert N == len(kept) and abs(got[k]["mean"] - kept.mean()) <= sr.mean_bar(N, sum_abs, total) * abs(kept.mean())
        assert abs(got[k]["std"] - kept.std()) <= sr.std_bar(N, kept.mean(), kept.std()) * kept.std()


def test_bins_are_the_constructors_linspace(gold):
    st = want_stats(gold, "twelve")
    p, e = stlib.bins(st)
    assert p.shape == e.shape == (255,) and p.dtype == np.float32 and p[0] == np.float32(st["pitch"]["min"]) and e[-1] == np.float32(st["energy"]["max"])
    assert np.array_equal(e, np.linspace(st["energy"]["min"], st["energy"]["max"], 255).astype(np.float32))
    assert stlib.bins({"energy": st["energy"]})[0] is None


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_stats.h")).read()
    hooks_block = re.search(r"#ifdef E2EST_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2est_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2EST_API [^;]*?\b(e2est_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(stlib.TEST_HOOK_SYMBOLS) and declared == sorted(stlib.EXPORTED_SYMBOLS)
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "stats", "stats.map")).read()
    assert re.search(r"global:\s*e2est_\*;\s*local:\s*\*;", vmap)
    n, k = len(declared), len(hook_syms)
    assert f"Exports: {n} entry points, and {k} more in the test build" in header and f"({n}, and {k} more in the test build)" in vmap
    assert f"libe2etts_stats.so` ({n} exports" in open(os.path.join(ROOT, "README.md")).read()

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(stlib.LIB_PATH) == declared, sorted(set(exported(stlib.LIB_PATH)) ^ set(declared))     # the product library: no test hook
    assert exported(stlib.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(stlib.LIB_PATH)                                                                        # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2est_abi_version() == stlib.ABI_VERSION == int(re.search(r"#define E2EST_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2EST_MAX_B", stlib.MAX_B), ("E2EST_MAX_ROW", stlib.MAX_ROW), ("E2EST_F0", stlib.F0), ("E2EST_ENERGY", stlib.ENERGY),
                      ("E2EST_PITCH", stlib.PITCH)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    assert stlib.ROW_DTYPE.itemsize == 72 and stlib.BLOCK_DTYPE.itemsize == 88
    import __graft_entry__ as g
    assert g.stats_hash() in lib.e2est_version().decode()
    assert any(os.path.basename(f) == "plan.h" for f in g.STATS["extra"]) and g.STATS in g.COMPANIONS and g.STATS["macro"] == "E2EST"
    plan = g.STATS["extra"][0]
    assert g.stats_hash() == g._marker_hash((g.STATS["src"], g.STATS["map"], g.STATS["hdr"], g.COMPANION_HDR, plan))    # plan.h is part of the hash
    # the other libraries are untouched: nothing of the companion is exported there
    from e2e_tts_amd import _lib, mel as mp, f0 as f0l, compare as cml
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH, mp.LIB_PATH, f0l.LIB_PATH, cml.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2est_" not in syms
    for f in ("stats.hip", "plan.h"):
        assert "getenv" not in open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "stats", f)).read()
    assert "hip" not in open(plan).read().lower().replace("__hipcc__", "").replace("hip-free", "").replace("stats.hip", "")


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and nothing was allocated."""
    P = C.c_void_p
    h = P()
    assert lib.e2est_create(0, None) == stlib.E_INVAL and lib.e2est_create(-1, C.byref(h)) == stlib.E_INVAL and not h.value
    assert b"device_id" in lib.e2est_last_error(None)
    assert lib.e2est_create(0, C.byref(h)) == stlib.E_OK and h.value
    x = np.zeros((2, 9), np.float32)
    lens = np.array([9, 4], np.int64)
    add = lambda kind, v, stride, ln, B, T: lib.e2est_add(h, kind, None if v is None else v.ctypes.data, stride, None if ln is None else ln.ctypes.data, B, T)   # noqa: E731
    assert add(3, x, 9, lens, 2, 9) == stlib.E_INVAL and b"kind" in lib.e2est_last_error(h) and add(-1, x, 9, lens, 2, 9) == stlib.E_INVAL
    assert add(1, None, 9, lens, 2, 9) == stlib.E_INVAL and add(1, x, 9, None, 2, 9) == stlib.E_INVAL
    assert add(1, x, 9, lens, 0, 9) == stlib.E_INVAL and add(1, x, 9, lens, 4097, 9) == stlib.E_INVAL and b"B must" in lib.e2est_last_error(h)
    assert add(1, x, 9, lens, 2, 0) == stlib.E_INVAL and add(1, x, 8, lens, 2, 9) == stlib.E_INVAL and b"row_stride" in lib.e2est_last_error(h)
    for ln, word in (([0, 4], b"at least 1"), ([9, 10], b"longer than T"), ([-1, 9], b"at least 1")):
        assert add(1, x, 9, np.array(ln, np.int64), 2, 9) == stlib.E_INVAL and word in lib.e2est_last_error(h) and b"row " in lib.e2est_last_error(h)
    big = np.array([5, 16385], np.int64)          # the values are not touched: the length is refused first
    assert add(1, x, 20000, big, 2, 20000) == stlib.E_INVAL and b"row 1" in lib.e2est_last_error(h) and b"E2EST_MAX_ROW" in lib.e2est_last_error(h)
    assert add(1, x, 9, lens, 2, 9) == stlib.E_INVAL and b"device memory" in lib.e2est_last_error(h)       # a host array is no row source
    out = np.zeros((2, 9), np.float32)
    norm = lambda ln, mean, std, o: lib.e2est_normalize(h, x.ctypes.data, 9, ln.ctypes.data, 2, 9, C.c_double(mean), C.c_double(std), None if o is None else o.ctypes.data)   # noqa: E731
    assert norm(lens, 0.0, 1.0, None) == stlib.E_INVAL and norm(lens, 0.0, 0.0, out) == stlib.E_INVAL and b"std" in lib.e2est_last_error(h)
    assert norm(lens, np.nan, 1.0, out) == stlib.E_INVAL and norm(lens, 0.0, -2.0, out) == stlib.E_INVAL and norm(lens, 0.0, 1e-60, out) == stlib.E_INVAL
    assert norm(np.array([9, 10], np.int64), 0.0, 1.0, out) == stlib.E_INVAL and b"[0, T]" in lib.e2est_last_error(h)
    assert norm(lens, 0.0, 1.0, out) == stlib.E_INVAL and b"device memory" in lib.e2est_last_error(h) and not out.any()
    rows = np.zeros(2, stlib.ROW_DTYPE)
    assert lib.e2est_fetch_rows(h, rows.ctypes.data) == stlib.E_STATE and lib.e2est_fetch_rows(h, None) == stlib.E_INVAL
    res = np.ones(3, stlib.BLOCK_DTYPE)
    assert lib.e2est_result(h, None) == stlib.E_INVAL and lib.e2est_result(h, res.ctypes.data) == stlib.E_OK and not res.view(np.uint8).any()   # all absent
    assert lib.e2est_reset(h) == stlib.E_OK and lib.e2est_sync(h) == stlib.E_OK and lib.e2est_device_bytes(h) == 0
    ms = (C.c_double * 3)()
    assert lib.e2est_profile_enable(h, 1) == stlib.E_OK and lib.e2est_profile_read(h, ms) == stlib.E_OK and list(ms) == [0.0, 0.0, 0.0]
    assert lib.e2est_profile_read(h, None) == stlib.E_INVAL
    lib.e2est_destroy(h)
    lib.e2est_destroy(None)
    for fn in (lib.e2est_sync, lib.e2est_stream, lib.e2est_reset):
        assert not fn(None) or fn(None) == stlib.E_INVAL
    st = stlib.CorpusStats()
    with pytest.raises(ValueError, match="lens is required"):
        st.add(energy=x)
    with pytest.raises(ValueError, match="nothing to add"):
        st.add(lens=lens)
    with pytest.raises(RuntimeError, match="rows before an add"):
        st.rows()
    assert st.result() == {}
    st.close()
