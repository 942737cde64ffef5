"""Recording conditioning, the parts that need no GPU: the plain-integer restatement (tests/condition_ref.py) against what audioop gave
(tests/golden/condition_cases.npz) and against audioop itself where it is importable, the tie cases of the definition, and the companion
library's C ABI -- its exports and the argument validation that runs before a device is opened."""
import ctypes as C
import hashlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import condition_cases as cc
import condition_ref as cr
from e2e_tts_amd import condition as cd

GOLDEN = os.path.join(ROOT, "tests", "golden", "condition_cases.npz")
TRIMS = (("none", None), ("reference", "reference"), ("both", "both"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_condition_hash() != g.condition_hash() or g.built_condition_hash(g.CONDITION["test_lib"]) != g.condition_hash():
        g.build()
    return cd.load_library()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return cc.cases()


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def test_ref_equals_the_recorded_audioop_results(golden, cases):
    n_ranges = 0
    for name, case in cases.items():
        for b, row in enumerate(case["rows"]):
            key = f"{name}/{b}"
            mono = row
            if case["channels"] == 2:
                mono = cr.downmix(row)
                assert np.array_equal(sha(mono), golden[f"{key}/tomono_sha"]), key
            assert cr.len_ms(len(mono), case["rate"]) == int(golden[f"{key}/len_ms"])
            rg = cr.detect_silence(mono, case["rate"])
            assert rg == golden[f"{key}/ranges"].tolist(), key
            n_ranges += len(rg)
            for gname, trim in TRIMS:
                r = cr.normalize(mono, case["rate"], trim, cc.TARGET_DBFS)
                assert [r["s_ms"], r["e_ms"], r["n_out"]] == golden[f"{key}/{gname}/span"].tolist(), (key, gname)
                assert r["sumsq"] == int(golden[f"{key}/{gname}/sumsq"])
                assert cd.rms_of(r["sumsq"], r["n_out"]) == int(golden[f"{key}/{gname}/rms"])
                assert r["gain"] == float(golden[f"{key}/{gname}/gain"]) == cd.loudness_gain(r["sumsq"], r["n_out"], cc.TARGET_DBFS)
                assert np.array_equal(sha(r["pcm"]), golden[f"{key}/{gname}/mul_sha"]), (key, gname)
                assert np.array_equal(sha(cr.normalize(mono, case["rate"], trim)["pcm"]), golden[f"{key}/{gname}/mul1_sha"])
    assert n_ranges >= 15   # the matrix does have silences, several rows with more than one range


def test_ref_equals_audioop_live():
    audioop = pytest.importorskip("audioop")
    rng = np.random.Generator(np.random.PCG64(3))
    thresh = 10 ** (-50 / 20) * 32768
    assert cd.threshold_k(-50) == cr.K_DEFAULT == 103 == math.floor(thresh)
    for trial in range(200):   # rms and the window test's integer form
        n = int(rng.integers(1, 600))
        x = (rng.integers(-32768, 32768, n) if trial % 2 else rng.integers(80, 130, n) * rng.choice([-1, 1], n)).astype(np.int16)
        r = audioop.rms(x.tobytes(), 2)
        assert r == cr.rms(x)
        assert (r <= thresh) == (cr.sumsq(x, 0, n) < (cr.K_DEFAULT + 1) ** 2 * n)
    for gain in (0.5, 1.7, 0.0, 1.0, 3.3333, 1e-3):
        x = rng.integers(-32768, 32768, 999).astype(np.int16)
        assert audioop.mul(x.tobytes(), 2, gain) == cr.mul(x, gain).tobytes()
    assert cr.mul([3, -3, 20000, -20000], 0.5).tolist() == [1, -2, 10000, -10000] and cr.mul([20000, -20000], 1.7).tolist() == [32767, -32768]
    st = rng.integers(-32768, 32768, (777, 2)).astype(np.int16)
    assert audioop.tomono(st.tobytes(), 2, 0.5, 0.5) == cr.downmix(st).tobytes()
    assert cr.downmix([[3, 4], [-3, -4]]).tolist() == [3, -4]
    for rate in (8000, 11025, 16000, 22050, 32000, 44100, 48000):   # pos against pydub's int(p * (rate / 1000.0))
        for p in list(range(0, 4000)) + [int(v) for v in rng.integers(0, 700000, 2000)]:
            assert cr.pos(p, rate) == int(p * (rate / 1000.0))


def test_threshold_ties():
    """Constant +-103 is silent, +-104 is not (rms <= k with k = 103)."""
    for rate in (8000, 22050):
        n = cr.pos(250, rate)
        for sign in (1, -1):
            assert cr.detect_silence(np.full(n, sign * 103, np.int16), rate) == [[0, 250]]
            assert cr.detect_silence(np.full(n, sign * 104, np.int16), rate) == []


def test_merge_at_exactly_W_and_split_at_W_plus_one(cases, golden):
    assert cr.ranges_of([5, 105]) == [[5, 205]] and cr.ranges_of([5, 106]) == [[5, 105], [106, 206]]
    assert cr.ranges_of([]) == [] and cr.ranges_of([0]) == [[0, 100]] and cr.ranges_of([0, 1, 2, 200, 300, 401]) == [[0, 102], [200, 400], [401, 501]]
    # on samples: the edge rows hold a silent start exactly W after its predecessor (merged) and one W + 1 after (split)
    for name, b in (("r8000", 4), ("r22050", 1)):
        x, rate = cases[name]["rows"][b], cases[name]["rate"]
        st = cr.silent_starts(x, rate)
        assert 1000 in st and 1100 in st and not any(1000 < s < 1100 for s in st)
        assert 1500 in st and 1601 in st and not any(1500 < s < 1601 for s in st)
        rg = cr.ranges_of(st)
        assert [1000, 1240] in rg and [1500, 1600] in rg and [1601, 1740] in rg
        assert rg == golden[f"{name}/{b}/ranges"].tolist()


def test_trailing_rule_all_silent_and_empty():
    rate = 8000
    rng = np.random.Generator(np.random.PCG64(1))
    loud = lambda ms: rng.integers(-8000, 8001, cr.pos(ms, rate)).astype(np.int16)   # noqa: E731
    quiet = lambda ms: np.zeros(cr.pos(ms, rate), np.int16)   # noqa: E731
    x = np.concatenate([quiet(150), loud(300), quiet(200)])
    assert cr.detect_silence(x, rate) == [[0, 150], [450, 650]]
    r = cr.normalize(x, rate, "reference")
    assert (r["s_ms"], r["e_ms"], r["n_out"]) == (150, 650, cr.pos(500, rate))   # the reference never trims the tail
    assert np.array_equal(r["pcm"], x[cr.pos(150, rate):])
    r = cr.normalize(x, rate, "both")
    assert (r["s_ms"], r["e_ms"], r["n_out"]) == (150, 450, cr.pos(300, rate)) and np.array_equal(r["pcm"], x[cr.pos(150, rate):cr.pos(450, rate)])
    r = cr.normalize(x, rate, None, -20.0)                                       # no trim: unsliced
    assert r["n_out"] == len(x) and r["ranges"] == [[0, 150], [450, 650]]
    x = np.concatenate([loud(100), quiet(200), loud(100)])                        # silence inside only: sliced [0, len_ms)
    assert cr.normalize(x, rate, "reference")["n_out"] == len(x) and cr.normalize(x, rate, "both")["n_out"] == len(x)
    for trim in ("reference", "both"):                                           # all silent: nothing is left, gain 1 (the reference: infinite)
        r = cr.normalize(quiet(400), rate, trim, -20.0)
        assert r["n_out"] == 0 and len(r["pcm"]) == 0 and r["gain"] == 1.0 and r["ranges"] == [[0, 400]]
    r = cr.normalize(quiet(50), rate, "reference", -20.0)                         # shorter than a window: no analysis; rms 0: gain 1
    assert r["ranges"] == [] and r["n_out"] == cr.pos(50, rate) and r["gain"] == 1.0
    assert cd.loudness_gain(0, 0, -20.0) == 1.0 and cd.loudness_gain(5, 100, -20.0) == 1.0 and cd.dbfs_of(0) == -math.inf
    # the overhang: pos(len_ms) > N is padded with zeros
    x = np.concatenate([quiet(120), loud(100)[:-3]])
    L = cr.len_ms(len(x), rate)
    assert cr.pos(L, rate) > len(x)
    r = cr.normalize(x, rate, "reference")
    assert r["n_out"] == cr.pos(L, rate) - cr.pos(r["s_ms"], rate) > len(x) - cr.pos(r["s_ms"], rate) and (r["pcm"][-3:] == 0).all()


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_condition.h")).read()
    hooks_block = re.search(r"#ifdef E2ECOND_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2econd_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2ECOND_API [^;]*?\b(e2econd_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(cd.TEST_HOOK_SYMBOLS) and declared == sorted(cd.EXPORTED_SYMBOLS)
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "condition", "condition.map")).read()
    assert re.search(r"global:\s*e2econd_\*;\s*local:\s*\*;", vmap)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(cd.LIB_PATH) == declared, sorted(set(exported(cd.LIB_PATH)) ^ set(declared))       # the product library: no test hook
    assert exported(cd.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(cd.LIB_PATH)                                                                        # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2econd_abi_version() == cd.ABI_VERSION == int(re.search(r"#define E2ECOND_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2ECOND_MAX_B", cd.MAX_B), ("E2ECOND_MIN_RATE", cd.MIN_RATE), ("E2ECOND_MAX_RATE", cd.MAX_RATE), ("E2ECOND_MAX_W", cd.MAX_W),
                      ("E2ECOND_TRIM_NONE", cd.TRIM_NONE), ("E2ECOND_TRIM_REFERENCE", cd.TRIM_REFERENCE), ("E2ECOND_TRIM_BOTH", cd.TRIM_BOTH),
                      ("E2ECOND_WANT_PCM", cd.WANT_PCM), ("E2ECOND_WANT_WAV", cd.WANT_WAV)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    import __graft_entry__ as g
    assert g.condition_hash() in lib.e2econd_version().decode()
    assert any(os.path.basename(f) == "plan.h" for f in g.CONDITION["extra"])
    # the other libraries are untouched: nothing of the companion is exported there, and the main library keeps its exports
    from e2e_tts_amd import _lib, aligner as al, mel as mp, resample as rs
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH, al.LIB_PATH, al.TEST_LIB_PATH, mp.LIB_PATH, mp.TEST_LIB_PATH, rs.LIB_PATH, rs.TEST_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2econd_" not in syms
    assert exported(_lib.LIB_PATH) == sorted(_lib.EXPORTED_SYMBOLS)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and the handle stays usable
    (device_bytes stays 0: nothing was allocated)."""
    P = C.c_void_p
    h = P()
    assert lib.e2econd_create(0, None) == cd.E_INVAL and lib.e2econd_create(-1, C.byref(h)) == cd.E_INVAL and not h.value
    assert b"e2econd_create" in lib.e2econd_last_error(None)
    assert lib.e2econd_create(0, C.byref(h)) == cd.E_OK and h.value
    B, n = 2, 64
    pcm = np.zeros((B, n), np.int16)
    rows = np.zeros(B, cd.ROW_DTYPE)
    ranges = np.full((B, 4, 2), -7, np.int32)

    def an(lens=None, a=pcm, stride=n, B=B, n=n, trim=cd.TRIM_REFERENCE, cap=4):
        arr = None if lens is None else np.asarray(lens, np.int64)
        return lib.e2econd_analyze(h, None if a is None else a.ctypes.data, stride, None if arr is None else arr.ctypes.data, B, n, trim, cap,
                                   rows.ctypes.data, ranges.ctypes.data)

    assert an() == cd.E_STATE and b"configure" in lib.e2econd_last_error(h)                        # not configured
    assert lib.e2econd_tile_starts(h) == 0
    for bad in ((999, 100, 103), (384001, 100, 103), (22050, 0, 103), (22050, 4097, 103), (22050, 100, -1), (22050, 100, 32768)):
        assert lib.e2econd_configure(h, *bad) == cd.E_INVAL, bad
    assert lib.e2econd_configure(h, 22050, 100, 103) == cd.E_OK and lib.e2econd_tile_starts(h) == 512
    assert an(a=None) == cd.E_INVAL
    assert an(B=0) == cd.E_INVAL and an(B=cd.MAX_B + 1) == cd.E_INVAL and an(n=0) == cd.E_INVAL and an(stride=n - 1) == cd.E_INVAL
    assert an(trim=3) == cd.E_INVAL and an(trim=-1) == cd.E_INVAL and an(cap=0) == cd.E_INVAL and an(cap=(1 << 20) + 1) == cd.E_INVAL
    assert an([64, 65]) == cd.E_INVAL and b"lens[1] = 65" in lib.e2econd_last_error(h)
    assert an([-1, 64]) == cd.E_INVAL and b"lens[0] = -1" in lib.e2econd_last_error(h)
    odd = np.zeros(2 * n + 1, np.int16)[1:].view(np.uint8)[1:]                                      # an int16 row at an odd address
    assert lib.e2econd_analyze(h, odd.ctypes.data, n, None, 1, n, 0, 1, None, None) == cd.E_INVAL and b"aligned" in lib.e2econd_last_error(h)
    assert (ranges == -7).all()
    gain = np.ones(B, np.float64)
    w = C.c_longlong(-7)
    assert lib.e2econd_apply(h, None, cd.WANT_PCM, None, None, 0, C.byref(w)) == cd.E_INVAL
    assert lib.e2econd_apply(h, gain.ctypes.data, 0, None, None, 0, C.byref(w)) == cd.E_INVAL and lib.e2econd_apply(h, gain.ctypes.data, 4, None, None, 0, C.byref(w)) == cd.E_INVAL
    out = np.zeros((B, n), np.float32)
    assert lib.e2econd_apply(h, gain.ctypes.data, cd.WANT_PCM, None, out.ctypes.data, n, C.byref(w)) == cd.E_INVAL    # wav_out without its bit
    assert lib.e2econd_apply(h, gain.ctypes.data, cd.WANT_PCM, None, None, 0, C.byref(w)) == cd.E_STATE and w.value == -7   # no analysis
    st = np.zeros((B, 2 * n), np.int16)
    assert lib.e2econd_downmix(h, None, 2 * n, B, n, None, 0) == cd.E_INVAL and lib.e2econd_downmix(h, st.ctypes.data, 2 * n - 1, B, n, None, 0) == cd.E_INVAL
    assert lib.e2econd_downmix(h, st.ctypes.data, 2 * n, 0, n, None, 0) == cd.E_INVAL
    assert lib.e2econd_downmix(h, st.ctypes.data, 2 * n, B, n, pcm.ctypes.data, n - 1) == cd.E_INVAL
    assert lib.e2econd_profile_read(h, None) == cd.E_INVAL
    assert not lib.e2econd_pcm_dev(h) and not lib.e2econd_wav_dev(h) and not lib.e2econd_mono_dev(h) and lib.e2econd_out_stride(h) == 0
    assert lib.e2econd_device_bytes(h) == 0 and lib.e2econd_sync(h) == cd.E_OK
    lib.e2econd_destroy(h)
    # the Python layer raises for the same, and for what it checks itself
    with pytest.raises(ValueError):
        cd.Conditioner(500)
    c = cd.Conditioner(22050)
    with pytest.raises(TypeError):
        c.analyze(np.zeros((1, 64), np.float32))
    with pytest.raises(ValueError):
        c.analyze(np.zeros((1, 64), np.int16), trim="tail")
    with pytest.raises(ValueError):
        c.analyze(np.zeros((2, 64), np.int16), lens=[64])
    with pytest.raises(ValueError):
        c.normalize(np.zeros((1, 64), np.int16), channels=3)
    with pytest.raises(ValueError):
        cd.normalize_signal(np.zeros((64, 2), np.int16), 22050)
    c.close()
    assert cd.max_ranges(22050 * 3, 22050, 100) == 29 and cd.len_ms(57342, 22050) == 2601
