"""The mel front-end, the parts that need no GPU: the numpy restatement (tests/mel_ref.py) against the reference's fixtures
(tools/make_mel_goldens.py), the two matrices of e2e_tts_amd/mel.py, the error bars (they pass a correct float32 evaluation and fail each
listed mistake), and the companion library's C ABI -- its exports and its argument validation, which runs before a device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import mel_ref as mr
from e2e_tts_amd import mel as mp

ALL = mr.FIXTURES + [mr.ALIGN_FIXTURE]
_CACHE = {}


def evaluated(name, dtype=np.float32, mut=None):
    """(mel, energy) of the restatement on a fixture, and the fixture's derived bars; computed once per (fixture, dtype, mistake)."""
    key = (name, np.dtype(dtype).name, mut)
    if key not in _CACHE:
        g = load_golden(name)
        audio = mr.fixture_audio(g)
        if ("bars", name) not in _CACHE:
            _CACHE[("bars", name)] = mr.derived_bars(audio, g["n_valid"], g)
        d = mr.dft64(int(g["n_fft"]), int(g["win_length"]), symmetric=mut == "sym_window").astype(dtype)
        mel, energy, lens = mr.mel_batch(audio.astype(dtype), g["n_valid"], d, g["mel_basis"].astype(dtype), int(g["hop"]), float(g["clip"]), dtype,
                                         None if mut == "sym_window" else mut)
        assert np.array_equal(lens, g["mel_lens"])
        _CACHE[key] = (mel, energy)
    return _CACHE[key], _CACHE[("bars", name)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_mel_hash() != g.mel_hash() or g.built_mel_hash(g.ML_TEST_LIB) != g.mel_hash():
        g.build()
    return mp.load_library()


@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_the_reference(name):
    """float64: the restatement IS the reference's formula (1e-9).  fp32: "equal to within the fixture's own fp32-vs-float64 error" is read as
    the triangle inequality on the means -- mean |restatement - reference fp32| <= mean |restatement - float64| + mean |reference fp32 -
    float64| <= (AGG_FACTOR + 1) x the fixture's own mean error, the first term being what the aggregate bar allows a correct float32
    evaluation.  The factor is derived, not fitted: the printed ratios are 0.7 to 2.0."""
    g = load_golden(name)
    lens = g["mel_lens"]
    (m64, e64), _ = evaluated(name, np.float64)
    assert mr.valid_stats(m64, g["mel64"], lens)[1] <= 1e-9
    assert mr.valid_stats(e64, g["energy64"], lens)[1] <= 1e-9 * max(1.0, float(g["energy64"].max()))
    # fp32 against the reference's fp32: both lie within their own error of the float64 values (the triangle inequality on the two means)
    (m32, e32), _ = evaluated(name)
    dm, de = mr.valid_stats(m32, g["mel32"], lens), mr.valid_stats(e32, g["energy32"], lens)
    print(f"{name}: restatement fp32 vs reference fp32 mel mean {dm[0]:.3e} max {dm[1]:.3e}; energy mean {de[0]:.3e} max {de[1]:.3e}; "
          f"{dm[0] / g['ref_err_mel'][0]:.2f} x / {de[0] / g['ref_err_energy'][0]:.2f} x the reference's own mean error")
    assert dm[0] <= (mr.AGG_FACTOR + 1) * g["ref_err_mel"][0] and de[0] <= (mr.AGG_FACTOR + 1) * g["ref_err_energy"][0]
    for b, n in enumerate(lens):
        assert not g["mel32"][b, n:].any() and not g["energy64"][b, n:].any()
    assert np.array_equal(lens, g["n_valid"] // int(g["hop"])) and g["mel32"].shape[1] == lens.max()
    for b, f0, f1 in g["zero_frames"]:   # the zero stretch: exactly log(1e-5) in fp32 in every channel
        assert f1 > f0 and (g["mel32"][b, f0:f1] == np.log(np.float32(1e-5))).all() and (m32[b, f0:f1] == np.log(np.float32(1e-5))).all()


@pytest.mark.parametrize("name", ALL)
def test_bars_pass_a_correct_float32_evaluation(name):
    (mel, energy), bars = evaluated(name)
    assert mr.check_against_fixture(mel, energy, load_golden(name), bars, label=name) == []


MISTAKES = ["drop_tap", "pad_half", "repeat_edge", "sym_window", "eps_after", "clamp_after", "energy_from_mel", "band_short"]


@pytest.mark.parametrize("mut", MISTAKES)
def test_bars_fail_each_mistake(mut):
    """Every mistake is caught on every fixture it can show on: a band cut one bin short needs a banded basis (the dense fixture's rows end at
    the last bin like any other, so it shows there too); 1e-9 added after the root shows where the signal is exactly zero."""
    for name in mr.FIXTURES:
        g = load_golden(name)
        if mut == "eps_after" and not len(g["zero_frames"]):
            continue
        (mel, energy), bars = evaluated(name, mut=mut)
        fails = mr.check_against_fixture(mel, energy, g, bars, label=f"{name} [{mut}]")
        assert fails, f"{mut} passes the bars on {name}"


def test_mel_filterbank_properties():
    """What can be derived without librosa (this function is parity-unpinned against librosa itself, see its docstring)."""
    assert abs(mp.hz_to_mel(1000.0) - 15.0) < 1e-12 and abs(mp.hz_to_mel(200.0) - 3.0) < 1e-12 and abs(mp.hz_to_mel(6400.0) - 42.0) < 1e-9
    assert abs(mp.hz_to_mel(1000.0 * np.exp(np.log(6.4) / 27.0)) - 16.0) < 1e-9          # one logarithmic step above 1 kHz
    f = np.array([0.0, 130.0, 999.0, 1000.0, 1001.0, 4321.0, 11025.0])
    assert np.allclose(mp.mel_to_hz(mp.hz_to_mel(f)), f, rtol=1e-12, atol=1e-9)
    for sr, n_fft, n_mels, fmin, fmax in ((22050, 1024, 80, 0.0, 8000.0), (48000, 2048, 80, 0.0, None), (4000, 128, 12, 0.0, 1500.0), (16000, 512, 40, 50.0, 7600.0)):
        w = mp.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        bins = n_fft // 2 + 1
        assert w.dtype == np.float32 and w.shape == (n_mels, bins) and (w >= 0).all()
        top = sr / 2.0 if fmax is None else fmax
        pts = mp.mel_frequencies(n_mels + 2, fmin, top)
        mels = mp.hz_to_mel(pts)
        assert np.allclose(np.diff(mels), (mels[-1] - mels[0]) / (n_mels + 1), rtol=1e-9) and abs(pts[0] - fmin) < 1e-9 and abs(pts[-1] - top) < 1e-6
        freqs = np.arange(bins) * sr / n_fft
        band = mp.band_table(w)
        for i in range(n_mels):
            a, b = band[i]
            assert b >= a, f"filter {i} is empty"
            assert (w[i, a:b + 1] > 0).all() and not w[i, :a].any() and not w[i, b + 1:].any()      # one contiguous band
            assert pts[i] < freqs[a] and freqs[b] < pts[i + 2]                                       # inside (f_i, f_{i+2})
            assert freqs[a] - sr / n_fft <= pts[i] and freqs[b] + sr / n_fft >= pts[i + 2]           # and all of it
            # the peak lies at the bin nearest the centre point, rising before it and falling after
            k = int(np.argmax(w[i]))
            assert abs(freqs[k] - pts[i + 1]) <= sr / n_fft
            assert (np.diff(w[i, a:k + 1]) > 0).all() and (np.diff(w[i, k:b + 1]) < 0).all()
            # area: the continuous triangle of height 2 / (f_{i+2} - f_i) has area 1 in Hz; sampled at the bins, sum * bin width = 1 up to the
            # quantisation, which is at most one bin's worth of the peak height on each slope
            height = 2.0 / (pts[i + 2] - pts[i])
            area = float(w[i].astype(np.float64).sum()) * sr / n_fft
            assert abs(area - 1.0) <= height * sr / n_fft, (i, area)
            # the weights are the triangle's values at the bin centres
            tri = height * np.maximum(0.0, np.minimum((freqs - pts[i]) / (pts[i + 1] - pts[i]), (pts[i + 2] - freqs) / (pts[i + 2] - pts[i + 1])))
            assert np.allclose(w[i], tri, rtol=1e-6, atol=1e-12)
    tiny = load_golden("mel_tiny_b3")["mel_basis"]
    assert not tiny[:, 49:].any() and np.array_equal(tiny, mp.mel_filterbank(4000, 128, 12, 0.0, 1500.0))   # bins above fmax: no weight anywhere


def test_dft_basis_against_rfft():
    rng = np.random.Generator(np.random.PCG64(3))
    for n_fft, win in ((64, 64), (128, 128), (128, 96), (1024, 1024), (1024, 800)):
        d = mp.dft_basis(n_fft, win)
        bins = n_fft // 2 + 1
        assert d.dtype == np.float32 and d.shape == (2 * bins, n_fft)
        w = np.zeros(n_fft)
        left = (n_fft - win) // 2
        w[left:left + win] = mp.hann_window(win)
        assert w[left] == 0.0 and abs(w[left + win // 2] - 1.0) < 1e-15           # periodic: the peak sits at win / 2, the last sample is not 0
        assert w[left + win - 1] > 0.0
        assert np.abs(d - mr.dft64(n_fft, win)).max() <= 2.0 ** -24               # rounded once from float64
        x = rng.standard_normal((5, n_fft))
        spec = x @ d.astype(np.float64).T
        ref = np.fft.rfft(x * w[None, :], axis=1)
        tol = 2.0 ** -23 * np.abs(x).sum(1).max()
        assert np.abs(spec[:, :bins] - ref.real).max() <= tol and np.abs(spec[:, bins:] + ref.imag).max() <= tol   # (sin rows: -imag of e^{-i...})
    with pytest.raises(ValueError):
        mp.dft_basis(64, 128)


def test_band_table_covers_exactly_the_non_zeros():
    for name in ALL:
        mb = load_golden(name)["mel_basis"]
        band = mp.band_table(mb)
        for m, (a, b) in enumerate(band):
            nz = np.flatnonzero(mb[m])
            assert a == nz[0] and b == nz[-1]
        mask = np.zeros(mb.shape, bool)
        for m, (a, b) in enumerate(band):
            mask[m, a:b + 1] = True
        assert not mb[~mask].any()
        if name == "mel_tiny_dense_b2":
            assert (band[:, 0] == 0).all() and (band[:, 1] == mb.shape[1] - 1).all()     # the degenerate band
        else:
            assert (mb[mask] != 0).all() and mask.sum() < 0.25 * mask.size               # triangles: contiguous, a small part of the matrix
    z = np.zeros((4, 9), np.float32)
    z[1, 3] = 1
    z[2, 0], z[2, 8] = 1, 1
    assert mp.band_table(z).tolist() == [[0, -1], [3, 3], [0, 8], [0, -1]]
    # the banded sum of the restatement is the dense sum, bit for bit: skipped terms are exact zeros
    g = load_golden("mel_tiny_b3")
    x = mr.fixture_audio(g)[0, :int(g["n_valid"][0])]
    d = mr.fixture_dft(g)
    a = mr.mel_row(x, d, g["mel_basis"], int(g["hop"]))
    b = mr.mel_row(x, d, g["mel_basis"], int(g["hop"]), band=mp.band_table(g["mel_basis"]))
    assert np.array_equal(a[0], b[0])


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_mel.h")).read()
    hooks_block = re.search(r"#ifdef E2EMEL_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2emel_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2EMEL_API [^;]*?\b(e2emel_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(mp.TEST_HOOK_SYMBOLS) and declared == sorted(mp.EXPORTED_SYMBOLS)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(mp.LIB_PATH) == declared, sorted(set(exported(mp.LIB_PATH)) ^ set(declared))       # the product library: no test hook
    assert exported(mp.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(mp.LIB_PATH)                                                                        # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2emel_abi_version() == mp.ABI_VERSION == int(re.search(r"#define E2EMEL_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2EMEL_MAX_B", mp.MAX_B), ("E2EMEL_MAX_MEL", mp.MAX_MEL), ("E2EMEL_F32", mp.F32), ("E2EMEL_I16", mp.I16)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    import __graft_entry__ as g
    assert g.mel_hash() in lib.e2emel_version().decode()
    # the other libraries are untouched by the companion: nothing of it is exported there, and the main library's source hash does not see it
    from e2e_tts_amd import _lib, aligner as al
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH, al.LIB_PATH, al.TEST_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2emel_" not in syms
    assert not any("mel" in os.path.basename(f) for f in __import__("glob").glob(os.path.join(g.CSRC, "*")) if os.path.isfile(f))


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and the handle stays usable
    (device_bytes stays 0: nothing was allocated)."""
    P = C.c_void_p
    h = P()
    for bad in ((0, 1000, 250, 80),      # hop % 32
                (0, 768, 256, 80),       # n_overlap 3
                (0, 256, 256, 80),       # n_overlap 1
                (0, 4096, 256, 80),      # n_overlap 16
                (0, 4096, 2048, 80),     # hop > 1024
                (0, 1024, 256, 82),      # n_mel % 4
                (0, 1024, 256, 0), (0, 1024, 256, mp.MAX_MEL + 4), (0, 1024, 0, 80), (0, -1024, 256, 80), (-1, 1024, 256, 80)):
        assert lib.e2emel_create(bad[0], bad[1], bad[2], bad[3], C.byref(h)) == mp.E_INVAL and not h.value, bad
        assert b"e2emel_create" in lib.e2emel_last_error(None)
    assert lib.e2emel_create(0, 1024, 256, 80, None) == mp.E_INVAL
    assert lib.e2emel_create(0, 1024, 256, 80, C.byref(h)) == mp.E_OK and h.value
    assert lib.e2emel_tile_frames(h) == 16
    B, n = 2, 2048
    audio = np.zeros((B, n), np.float32)
    mel, energy, lens = np.zeros((B, 8, 80), np.float32), np.zeros((B, 8), np.float32), np.zeros(B, np.int64)
    T = C.c_int(-7)

    def fwd(nv, a=audio, dtype=mp.F32, stride=n, B=B, n=n):
        arr = None if nv is None else np.asarray(nv, np.int64)   # (kept alive over the call)
        return lib.e2emel_forward(h, None if a is None else a.ctypes.data, dtype, stride, None if arr is None else arr.ctypes.data, B, n,
                                  mel.ctypes.data, energy.ctypes.data, lens.ctypes.data, C.byref(T))

    assert fwd(None, a=None) == mp.E_INVAL
    assert fwd(None, dtype=2) == mp.E_INVAL and fwd(None, dtype=-1) == mp.E_INVAL
    assert fwd(None, B=0) == mp.E_INVAL and fwd(None, B=mp.MAX_B + 1) == mp.E_INVAL
    assert fwd(None, n=0) == mp.E_INVAL and fwd(None, stride=n - 1) == mp.E_INVAL
    assert fwd([2048, 2049]) == mp.E_INVAL and b"n_valid[1] = 2049" in lib.e2emel_last_error(h)       # longer than n
    assert fwd([384, 2048]) == mp.E_INVAL and b"n_valid[0] = 384" in lib.e2emel_last_error(h)         # = (n_fft - hop) / 2: cannot be reflected
    assert fwd([2048, 0]) == mp.E_INVAL and fwd([-5, 2048]) == mp.E_INVAL
    assert fwd(None, n=1 << 40, stride=1 << 40) == mp.E_INVAL and b"too large" in lib.e2emel_last_error(h)
    assert fwd(None) == mp.E_STATE and fwd([385, 2048]) == mp.E_STATE                                 # valid arguments: call order (nothing loaded)
    assert T.value == -7 and not mel.any()
    # loading: NULLs and the clip
    d, mb = mp.dft_basis(1024), mp.mel_filterbank(22050, 1024, 80, 0.0, 8000.0)
    assert lib.e2emel_load(h, None, mb.ctypes.data, 1e-5) == mp.E_INVAL and lib.e2emel_load(h, d.ctypes.data, None, 1e-5) == mp.E_INVAL
    for clip in (0.0, -1e-5, float("nan"), float("inf")):
        assert lib.e2emel_load(h, d.ctypes.data, mb.ctypes.data, clip) == mp.E_INVAL and b"clip_val" in lib.e2emel_last_error(h)
    assert lib.e2emel_profile_read(h, None) == mp.E_INVAL
    assert not lib.e2emel_mel_dev(h) and not lib.e2emel_energy_dev(h)                                 # nothing resident
    assert lib.e2emel_device_bytes(h) == 0
    assert fwd(None) == mp.E_STATE and lib.e2emel_sync(h) == mp.E_OK                                  # still usable
    lib.e2emel_destroy(h)
    # a geometry with n_overlap 2: a row of (n_fft - hop) / 2 < n_valid < hop samples has no frame
    assert lib.e2emel_create(0, 64, 32, 12, C.byref(h)) == mp.E_OK
    a2 = np.zeros((1, 64), np.float32)
    nv2 = np.array([20], np.int64)
    assert lib.e2emel_forward(h, a2.ctypes.data, mp.F32, 64, nv2.ctypes.data, 1, 64, None, None, None, None) == mp.E_INVAL
    assert b"one frame" in lib.e2emel_last_error(h)
    lib.e2emel_destroy(h)
    assert [lib.e2emel_tile_frames(x) for x in (None,)] == [0]
    for n_fft, hop, tile in ((2048, 512, 8), (8192, 1024, 2), (128, 32, 16)):                         # the tail's tile by the LDS a row of magnitudes needs
        assert mp.MelFrontend(n_fft, hop, 80).tile_frames == tile
    with pytest.raises(ValueError):
        mp.MelFrontend(1000, 250, 80)
    with pytest.raises(ValueError):
        mp.MelFrontend(1024, 256, 80).load(mp.dft_basis(512), mb)
