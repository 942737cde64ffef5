"""The pitch tracker, the parts that need no GPU: the float64 reference (tests/f0_ref.py) against its committed tracks and against a known
contour, the margins of every committed case under the caps the GPU tests rely on, the targets restatement against models.f0_targets,
extract_f0's length contract, and the companion library's C ABI -- its exports and the refusals that come before a device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import f0_cases as fc
import f0_ref as fr
from e2e_tts_amd import config as cfgmod, f0 as f0lib
from e2e_tts_amd.models import extract_f0, f0_targets, f0_to_coarse

_REF = {}


def refs(name):
    if name not in _REF:
        _REF[name] = fc.reference(fc.build(name))
    return _REF[name]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_f0_hash() != g.f0_hash() or g.built_f0_hash(g.F0["test_lib"]) != g.f0_hash():
        g.build()
    return f0lib.load_library()


@pytest.mark.parametrize("name", list(fc.CASES))
def test_reference_gives_its_committed_tracks(name):
    g = load_golden("f0_cases")
    for b, r in enumerate(refs(name)):
        T = r["T"]
        assert T == g[name + ".frames"][b]
        assert np.array_equal(r["index"], g[name + ".index"][b, :T])
        assert np.array_equal(r["f0"] == 0, g[name + ".f0"][b, :T] == 0)
        assert np.allclose(r["f0"], g[name + ".f0"][b, :T], rtol=1e-9, atol=0)
        m = g[name + ".path_margin"][b]
        assert r["path_margin"] == m or abs(r["path_margin"] - m) <= 1e-9 * abs(m)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_committed_cases_pass_the_seed_filter(name):
    """With the reference alone: at most 5 % of the frames left out of the candidate comparison, every path margin at least 1e-9, the rows
    the end-to-end test compares have a path gap above their budget, and there is such a row."""
    rs = refs(name)
    share, margin, rows, close = fc.verdict(rs)
    print(f"{name}: frames left out {share:.3f}, smallest path margin {margin:.3e}, rows compared {rows}, smallest maximum margin "
          f"{min(float(r['max_margin'].min(initial=np.inf)) for r in rs):.3e}, largest r bar {max(float(r['bar_r'].max(initial=0)) for r in rs):.3e}")
    assert share <= fc.MAX_LEFT_OUT and margin >= fc.MIN_PATH_MARGIN and rows and not close
    assert fc.accepts(rs) and fc.first_good_seed(name) == fc.SEEDS[name]


def test_cases_cover_the_corners():
    K = fr.DEFAULTS["max_candidates"]
    mixed, short, edges, pcm = (refs(n) for n in ("mixed_22k", "short_48k", "edges_16k", "pcm_22k"))
    assert mixed[1]["n_maxima"].max() > K - 1 and np.isfinite(mixed[1]["cut_margin"]).any()      # noise: the K - 1 cut is taken
    assert (mixed[2]["n_maxima"][3:-3] <= 5).all() and (mixed[2]["f0"][3:-3] > 0).all()          # a sine: few maxima, voiced
    assert (mixed[0]["f0"] == 0).any() and (mixed[0]["f0"] > 0).any()                            # silent stretches and tone
    assert [r["T"] for r in short][1:] == [1, 3] and fc.build("short_48k")["n_valid"][2] < short[0]["W"]
    assert edges[2]["g"] == 0 and not edges[2]["f0"].any() and not edges[2]["valid"].any()       # the all-zero row
    assert abs(np.median(edges[0]["f0"][2:-2]) - 81.0) < 0.2 and abs(np.median(edges[1]["f0"][2:-2]) - 740.0) < 0.5
    assert fc.build("pcm_22k")["wavs"].dtype == np.int16
    for name in fc.CASES:                                                                        # a tile boundary inside a row
        c = fc.build(name)
        F = {22050: 16, 16000: 16, 48000: 4}[c["sr"]]
        assert (c["n_valid"] // c["hop"]).max() > F


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_follows_a_known_contour(seed):
    """A five-harmonic tone whose f0 glides and vibrates: median relative error of the voiced frames <= 1e-3 (a prototype of this
    definition measured 0.7e-4 to 1.1e-4; the bar leaves a factor of ten)."""
    sr, hop, n = 22050, 256, 26460
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f = (150.0 + 40.0 * seed) * (1.0 + 0.1 * t + 0.02 * np.sin(2 * np.pi * 5.0 * t + rng.uniform(0, 6.28)))
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = (0.3 * sum(a * np.sin((k + 1) * ph + rng.uniform(0, 6.28)) for k, a in enumerate([1.0, 0.5, 0.35, 0.2, 0.1])) / 2.15 + 0.002 * rng.standard_normal(n)).astype(np.float32)
    r = fr.track(x, n, sr, hop)
    c = np.arange(r["T"]) * hop + hop // 2
    inner = slice(3, r["T"] - 3)                                            # whole windows
    assert (r["f0"][inner] > 0).all()
    err = np.abs(r["f0"][inner] / f[c][inner] - 1.0)
    print(f"seed {seed}: median relative error {np.median(err):.2e}")
    assert np.median(err) <= 1e-3


def test_float32_evaluation_stays_inside_the_bars():
    """The derived bar of r holds for a float32 numpy evaluation in the header's order (chunks of 32, then the chunk sums), with room."""
    c = fc.build("mixed_22k")
    sr, hop = c["sr"], c["hop"]
    for b in (0, 1):
        A = fr.acf(c["wavs"][b], int(c["n_valid"][b]), sr, hop)
        w, rw = (v.astype(np.float32) for v in fr.tables(sr, 80.0))
        win = fr.frame_windows(c["wavs"][b], int(c["n_valid"][b]), sr, hop, 80.0)
        W = A["W"]
        for t in (0, 7, A["T"] - 1):
            if not A["valid"][t]:
                continue
            xs = win[t].astype(np.float32)
            m = np.float32(win[t].sum() / W)
            a = np.zeros((W + 31) // 32 * 32 + A["NL"], np.float32)
            a[:W] = (xs - m) * w
            r32 = np.zeros(A["NL"], np.float32)
            for tau in range(A["NL"]):
                prod = (a[:(W + 31) // 32 * 32] * a[tau:tau + (W + 31) // 32 * 32]).reshape(-1, 32)
                chunks = np.zeros(prod.shape[0], np.float32)
                for k in range(32):
                    chunks = (chunks + prod[:, k]).astype(np.float32)
                tot = np.float32(0)
                for v in chunks:
                    tot = np.float32(tot + v)
                r32[tau] = tot
            r32 = r32 / (r32[0] * rw)
            assert (np.abs(r32.astype(np.float64) - A["r"][t]) <= A["bar_r"][t]).all()


def test_targets_restatement_equals_f0_targets():
    rng = np.random.default_rng(5)
    stats = cfgmod.DEFAULT_STATS
    tracks = [np.where(rng.random(60) > 0.4, rng.uniform(80, 400, 60), 0.0), np.zeros(17), np.r_[np.zeros(9), 210.5, np.zeros(9)], rng.uniform(90, 300, 12),
              np.r_[0.0, 0.0, 100.0, 0.0, 0.0, 0.0, 317.25, 0.0]]
    for tr in tracks:
        tr = tr.astype(np.float32).astype(np.float64)
        for mode in ("linear", "log"):
            a, au = f0_targets(tr, stats, mode, 1e-9)
            b, bu = fr.targets(tr, stats["f0"]["mean"], stats["f0"]["std"], mode, 1e-9)
            assert np.array_equal(a, b) and np.array_equal(au, bu)      # np.interp's arithmetic, bit for bit


def test_extract_f0_length_contract_and_coarse_bins():
    x = np.zeros(256 * 10 + 100, np.float32)
    with pytest.raises(ValueError, match="10 mel frames"):
        extract_f0(x, 11, 22050, 256)                                    # refused before a device is touched
    with pytest.raises(ValueError, match="one utterance"):
        extract_f0(x[None], 10, 22050, 256)
    f0 = np.array([0.0, 50.0, 80.0, 220.0, 750.0, 1100.0, 5000.0])
    coarse = f0_to_coarse(f0)
    assert coarse.dtype.kind == "i" and coarse[0] == 1 and coarse[1] == 1 and coarse[5] == 255 and coarse[6] == 255
    assert (np.diff(coarse) >= 0).all() and 1 < coarse[3] < 255
    mel = 1127 * np.log(1 + 220.0 / 700)
    lo, hi = 1127 * np.log(1 + 50.0 / 700), 1127 * np.log(1 + 1100.0 / 700)
    assert coarse[3] == int(np.rint((mel - lo) * 254 / (hi - lo) + 1))


def test_window_tables_are_the_references():
    for sr in (16000, 22050, 48000):
        w, rw = f0lib.window_tables(sr, 80.0)
        w2, rw2 = fr.tables(sr, 80.0)
        W, tau_min, tau_max = f0lib.geometry(sr, 80.0, 750.0)
        assert (W, tau_min, tau_max) == fr.geometry(sr, 80.0, 750.0) and w.shape == (W,) and rw.shape == (tau_max + 2,)
        assert w.dtype == rw.dtype == np.float32 and rw[0] == 1.0
        assert np.abs(w.astype(np.float64) - w2).max() <= 2.0 ** -24 and np.abs(rw.astype(np.float64) - rw2).max() <= 2.0 ** -23   # two float64 sums, rounded once
    assert f0lib.DEFAULTS == fr.DEFAULTS


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_f0.h")).read()
    hooks_block = re.search(r"#ifdef E2EF0_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2ef0_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2EF0_API [^;]*?\b(e2ef0_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(f0lib.TEST_HOOK_SYMBOLS) and declared == sorted(f0lib.EXPORTED_SYMBOLS)
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "f0", "f0.map")).read()
    assert re.search(r"global:\s*e2ef0_\*;\s*local:\s*\*;", vmap)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(f0lib.LIB_PATH) == declared, sorted(set(exported(f0lib.LIB_PATH)) ^ set(declared))     # the product library: no test hook
    assert exported(f0lib.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(f0lib.LIB_PATH)                                                                        # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2ef0_abi_version() == f0lib.ABI_VERSION == int(re.search(r"#define E2EF0_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2EF0_MAX_B", f0lib.MAX_B), ("E2EF0_MAX_K", f0lib.MAX_K), ("E2EF0_MIN_RATE", f0lib.MIN_RATE), ("E2EF0_MAX_RATE", f0lib.MAX_RATE),
                      ("E2EF0_F32", f0lib.F32), ("E2EF0_I16", f0lib.I16), ("E2EF0_LINEAR", f0lib.LINEAR), ("E2EF0_LOG", f0lib.LOG)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    assert C.sizeof(f0lib.CParams) == 72
    import __graft_entry__ as g
    assert g.f0_hash() in lib.e2ef0_version().decode()
    assert any(os.path.basename(f) == "plan.h" for f in g.F0["extra"])
    # the other libraries are untouched: nothing of the companion is exported there
    from e2e_tts_amd import _lib, aligner as al, mel as mp, resample as rsl, condition as cdl
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH, al.LIB_PATH, mp.LIB_PATH, rsl.LIB_PATH, cdl.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2ef0_" not in syms
    # no getenv in the new sources
    for f in ("f0.hip", "plan.h"):
        assert "getenv" not in open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "f0", f)).read()


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and nothing was allocated."""
    P = C.c_void_p
    h = P()
    assert lib.e2ef0_create(0, 22050, 256, None) == f0lib.E_INVAL and lib.e2ef0_create(-1, 22050, 256, C.byref(h)) == f0lib.E_INVAL and not h.value
    assert lib.e2ef0_create(0, 999, 256, C.byref(h)) == f0lib.E_INVAL and lib.e2ef0_create(0, 22050, 0, C.byref(h)) == f0lib.E_INVAL
    assert b"e2ef0_create" in lib.e2ef0_last_error(None)
    assert lib.e2ef0_create(0, 22050, 256, C.byref(h)) == f0lib.E_OK and h.value
    w, rw = f0lib.window_tables(22050, 80.0)

    def params(**kw):
        d = {**f0lib.DEFAULTS, **kw}
        return f0lib.CParams(kw.pop("struct_size", C.sizeof(f0lib.CParams)), *(float(d[k]) for k in list(f0lib.DEFAULTS)[:-1]), int(d["max_candidates"]))

    def configure(p, w_=w, rw_=rw):
        return lib.e2ef0_configure(h, C.byref(p) if p is not None else None, None if w_ is None else w_.ctypes.data, None if rw_ is None else rw_.ctypes.data)

    assert configure(None) == f0lib.E_INVAL and configure(params(), None) == f0lib.E_INVAL and configure(params(), w, None) == f0lib.E_INVAL
    bad = params()
    bad.struct_size = 64
    assert configure(bad) == f0lib.E_INVAL and b"struct_size" in lib.e2ef0_last_error(h)
    for kw, word in ((dict(max_candidates=17), b"max_candidates"), (dict(max_candidates=1), b"max_candidates"), (dict(silence_threshold=0.0), b"silence_threshold"),
                     (dict(voicing_threshold=float("nan")), b"voicing_threshold"), (dict(octave_jump_cost=-1.0), b"octave_jump_cost"),
                     (dict(ceiling=30000.0), b"tau_min"), (dict(floor=0.0), b"floor"), (dict(floor=800.0), b"floor"), (dict(floor=10.0), b"LDS")):
        assert configure(params(**kw)) == f0lib.E_INVAL and word in lib.e2ef0_last_error(h), kw
    for table, i, v in (("w", 3, np.nan), ("w", 5, 1.5), ("w", 0, -0.1), ("rw", 0, 0.999), ("rw", 9, 0.0), ("rw", 9, np.inf)):
        w2, rw2 = w.copy(), rw.copy()
        (w2 if table == "w" else rw2)[i] = v
        assert configure(params(), w2, rw2) == f0lib.E_INVAL, (table, i, v)
    x = np.zeros((2, 4096), np.float32)
    nv = np.array([4096, 4096], np.int64)
    T = C.c_int(-1)
    fwd = lambda *a: lib.e2ef0_forward(h, *a, None, None, C.byref(T))   # noqa: E731
    assert fwd(x.ctypes.data, f0lib.F32, 4096, nv.ctypes.data, 2, 4096) == f0lib.E_STATE and b"configure" in lib.e2ef0_last_error(h)
    assert fwd(None, f0lib.F32, 4096, nv.ctypes.data, 2, 4096) == f0lib.E_INVAL and fwd(x.ctypes.data, 2, 4096, nv.ctypes.data, 2, 4096) == f0lib.E_INVAL
    assert lib.e2ef0_targets(h, 0.0, 1.0, 0, 1e-9, None, None) == f0lib.E_STATE
    assert lib.e2ef0_targets(h, 0.0, 0.0, 0, 1e-9, None, None) == f0lib.E_INVAL and lib.e2ef0_targets(h, 0.0, 1.0, 2, 1e-9, None, None) == f0lib.E_INVAL
    assert lib.e2ef0_targets(h, 0.0, 1.0, 1, -1.0, None, None) == f0lib.E_INVAL
    assert not lib.e2ef0_f0_dev(h) and not lib.e2ef0_target_f0_dev(h) and not lib.e2ef0_target_uv_dev(h) and lib.e2ef0_tile_frames(h) == 0
    assert lib.e2ef0_device_bytes(h) == 0 and T.value == -1
    assert lib.e2ef0_window(22050, 256, 80.0, 750.0) == 827 and lib.e2ef0_lags(22050, 256, 80.0, 750.0) == 277 and lib.e2ef0_tau_min(22050, 256, 80.0, 750.0) == 30
    assert lib.e2ef0_window(48000, 512, 80.0, 750.0) == 1801 and lib.e2ef0_window(48000, 512, 40.0, 750.0) == f0lib.E_INVAL
    ms = (C.c_double * 3)()
    assert lib.e2ef0_profile_enable(h, 1) == f0lib.E_OK and lib.e2ef0_profile_read(h, ms) == f0lib.E_OK and list(ms) == [0.0, 0.0, 0.0]
    assert lib.e2ef0_profile_read(h, None) == f0lib.E_INVAL and lib.e2ef0_sync(h) == f0lib.E_OK
    lib.e2ef0_destroy(h)
    lib.e2ef0_destroy(None)
    for fn in (lib.e2ef0_sync, lib.e2ef0_stream, lib.e2ef0_f0_dev):
        assert not fn(None) or fn(None) == f0lib.E_INVAL
    with pytest.raises(ValueError, match="unknown parameters"):
        f0lib.PitchTracker(22050, 256, pitch_floor=80)
