"""The resampler, the parts that need no GPU: the numpy restatement (tests/resample_ref.py) against scipy.signal.resample_poly, the
derived error bar (it passes a correct float32 evaluation and fails each listed mistake), the default filter design, the stream
bookkeeping, and the companion library's C ABI -- its exports and the argument validation that runs before a device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import resample_ref as rr
from e2e_tts_amd import resample as rs

# (src rate, dst rate) -> (L, M): the six ratios of the arithmetic's contract
SCIPY_RATIOS = [(441, 160), (147, 320), (1, 2), (2, 1), (147, 160), (7, 3)]
# the rate pairs the project serves, with (L, M, taps, P) of the default design
RATE_PAIRS = [((22050, 8000), (160, 441, 14113, 89)), ((22050, 16000), (320, 441, 14113, 45)), ((22050, 48000), (320, 147, 10241, 33)),
              ((48000, 8000), (1, 6, 193, 193)), ((48000, 22050), (147, 320, 10241, 70))]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_resample_hash() != g.resample_hash() or g.built_resample_hash(g.RS_TEST_LIB) != g.resample_hash():
        g.build()
    return rs.load_library()


@pytest.mark.parametrize("src,dst", SCIPY_RATIOS)
def test_definition_equals_scipy_resample_poly(src, dst):
    signal = pytest.importorskip("scipy.signal")
    taps, L, M = rs.design(src, dst, zeros=2 if (src, dst) == (7, 3) else 16)
    assert (L, M) == (dst, src)
    for n in (1, 37, 1000, 1001):
        x = rr.make_signal(n, seed=n)
        y = rr.resample_f64(x, taps, L, M)
        ref = signal.resample_poly(x.astype(np.float64), L, M, window=taps.astype(np.float64) / L)   # scipy multiplies a given window by `up`
        assert y.shape == ref.shape == (rr.n_out(n, L, M),)
        assert np.abs(y - ref).max() <= 1e-12
    xi = rr.make_signal(500, seed=5, dtype=np.int16)   # int16 input is the same signal / 32768
    assert np.array_equal(rr.resample_f64(xi, taps, L, M), rr.resample_f64((xi / 32768.0).astype(np.float32), taps, L, M))


# ((src, dst), zeros of the design, samples): L = 3, 2, 160, 147; then the two ratios with L = 1
CASES = [((7, 3), 2, 1500), ((1, 2), 16, 1200), ((441, 160), 16, 1500), ((320, 147), 16, 800)]
ONE_PHASE = [((2, 1), 16, 1200), ((6, 1), 16, 1500)]


@pytest.mark.parametrize("ratio,zeros,n", CASES + ONE_PHASE)
def test_bar_passes_the_float32_chain(ratio, zeros, n):
    taps, L, M = rs.design(*ratio, zeros=zeros)
    for dtype in (np.float32, np.int16):
        x = rr.make_signal(n, seed=2, dtype=dtype)
        y64, y32, b = rr.resample_f64(x, taps, L, M), rr.resample_f32(x, taps, L, M), rr.bar(x, taps, L, M)
        worst = float((np.abs(y32 - y64) / np.maximum(b, 1e-300)).max())
        print(f"{L}/{M} {np.dtype(dtype).name}: worst |fp32 chain - float64| / bar = {worst:.3f}")
        assert rr.failing_fraction(y32, y64, b) == 0.0


# (L = 1 has one phase: a phase off by one is the same phase, so the mistakes are shown on the ratios with L > 1)
@pytest.mark.parametrize("ratio,zeros,n", CASES)
@pytest.mark.parametrize("mut", rr.MUTATIONS)
def test_bar_fails_each_mistake(ratio, zeros, n, mut):
    taps, L, M = rs.design(*ratio, zeros=zeros)
    x = rr.make_signal(n, seed=2)
    y64, b = rr.resample_f64(x, taps, L, M), rr.bar(x, taps, L, M)
    frac = rr.failing_fraction(rr.resample_f32(x, taps, L, M, mut=mut), y64, b)
    print(f"{L}/{M} {mut}: {100 * frac:.1f} % of samples outside the bar")
    assert frac >= 0.01


def test_floor_for_ceil_in_n_out_fails_on_length():
    taps, L, M = rs.design(7, 3, zeros=2)
    x = rr.make_signal(100, seed=1)
    assert (100 * L) % M != 0
    y64 = rr.resample_f64(x, taps, L, M)
    short = rr.resample_f32(x, taps, L, M, ms=np.arange((100 * L) // M))
    assert len(short) == len(y64) - 1 and rr.failing_fraction(short, y64, rr.bar(x, taps, L, M)) == 1.0


@pytest.mark.parametrize("rates,expect", RATE_PAIRS)
def test_default_design_meets_its_conditions(rates, expect):
    taps, L, M = rs.design(*rates)
    assert taps.dtype == np.float32 and (L, M, taps.size, rr.taps_per_output(taps.size, L)) == expect
    assert np.array_equal(taps, taps[::-1]) and abs(float(taps.astype(np.float64).sum()) - L) < 1e-4 * L   # linear phase, gain L
    r = rs.response(taps, L, M)
    print(f"{rates[0]} -> {rates[1]}: ripple {r['ripple_db']:.5f} dB, stopband {r['stopband_db']:.1f} dB, phase DC error {r['phase_dc_err']:.2e}")
    assert r["ripple_db"] <= 0.01 and r["stopband_db"] <= -80.0 and r["phase_dc_err"] <= 1e-4


def test_design_and_ratio_arguments():
    assert rs.ratio(22050, 16000) == (320, 441) and rs.ratio(48000, 48000) == (1, 1) and rs.ratio(44100, 22050) == (1, 2)
    with pytest.raises(ValueError):
        rs.ratio(0, 16000)
    with pytest.raises(ValueError):
        rs.design(2, 1, zeros=0)
    assert int(rs.n_out(100, 3, 7)) == 43 and rs.n_out(np.array([0, 1, 7]), 3, 7).tolist() == [0, 1, 3]


def test_stream_formulas_emit_every_output_once():
    """The Python restatement of plan.h's stream bookkeeping: emitting by E' over random chunkings gives exactly ceil(N L / M) outputs, each
    once and in order, computable from the samples that have arrived, with a history that never starts above k_lo of the next output."""
    rng = np.random.Generator(np.random.PCG64(9))
    for L, M, half in ((160, 441, 7056), (320, 147, 5120), (1, 6, 96), (3, 7, 14), (2, 1, 32), (5, 3, 0), (1, 6, 0)):
        for trial in range(6):
            total = int(rng.integers(1, 4000))
            N = E = kbuf = 0
            out = []
            while True:
                c = min(int(rng.integers(0, 700)) if trial else 1, total - N)
                flush = trial % 2 == 1   # odd trials end with an empty push that carries `last`
                last = N + c == total and (not flush or c == 0)
                keep = max(kbuf, min(rr.history_start(E, L, M, half), N))
                assert kbuf <= keep <= N
                N += c
                E2 = rr.emitted(N, L, M, half, last)
                for m in range(E, E2):
                    lo, hi = rr.k_lo(m, L, M, half), rr.k_hi(m, L, M, half)
                    assert max(lo, 0) >= keep or lo > hi, "the history was trimmed above a sample this output reads"
                    assert last or hi <= N - 1, "an output was emitted before its last sample arrived"
                out.extend(range(E, E2))
                if not last:
                    assert rr.k_hi(E2, L, M, half) >= N, "an output that could be computed was held back"
                E, kbuf = E2, keep
                if last:
                    break
            assert out == list(range(rr.n_out(total, L, M)))


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_resample.h")).read()
    hooks_block = re.search(r"#ifdef E2ERS_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2ers_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2ERS_API [^;]*?\b(e2ers_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(rs.TEST_HOOK_SYMBOLS) and declared == sorted(rs.EXPORTED_SYMBOLS)
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "resample", "resample.map")).read()
    assert re.search(r"global:\s*e2ers_\*;\s*local:\s*\*;", vmap)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(rs.LIB_PATH) == declared, sorted(set(exported(rs.LIB_PATH)) ^ set(declared))       # the product library: no test hook
    assert exported(rs.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(rs.LIB_PATH)                                                                        # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2ers_abi_version() == rs.ABI_VERSION == int(re.search(r"#define E2ERS_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2ERS_MAX_B", rs.MAX_B), ("E2ERS_MAX_RATIO", rs.MAX_RATIO), ("E2ERS_MAX_PHASE_TAPS", rs.MAX_PHASE_TAPS), ("E2ERS_F32", rs.F32),
                      ("E2ERS_I16", rs.I16)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    import __graft_entry__ as g
    assert g.resample_hash() in lib.e2ers_version().decode()
    # plan.h is part of the companion's hash; the main library's source hash does not see the companion
    assert any(os.path.basename(f) == "plan.h" for f in g.RESAMPLE["extra"])
    assert not any("resample" in os.path.basename(f) or "plan" in os.path.basename(f) for f in __import__("glob").glob(os.path.join(g.CSRC, "*")) if os.path.isfile(f))
    # the other libraries are untouched: nothing of the companion is exported there
    from e2e_tts_amd import _lib, aligner as al, mel as mp
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH, al.LIB_PATH, al.TEST_LIB_PATH, mp.LIB_PATH, mp.TEST_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2ers_" not in syms


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and the handle stays usable
    (device_bytes stays 0: nothing was allocated)."""
    P = C.c_void_p
    h = P()
    assert lib.e2ers_create(0, None) == rs.E_INVAL and lib.e2ers_create(-1, C.byref(h)) == rs.E_INVAL and not h.value
    assert b"e2ers_create" in lib.e2ers_last_error(None)
    assert lib.e2ers_create(0, C.byref(h)) == rs.E_OK and h.value
    taps = rs.design(2, 1)[0]
    ptr = taps.ctypes.data

    def load(t, n_taps, L, M):
        return lib.e2ers_load(h, t, n_taps, L, M)

    assert load(None, 65, 2, 1) == rs.E_INVAL
    assert load(ptr, 64, 2, 1) == rs.E_INVAL and b"odd" in lib.e2ers_last_error(h)
    assert load(ptr, 0, 2, 1) == rs.E_INVAL and load(ptr, -5, 2, 1) == rs.E_INVAL
    assert load(ptr, 65, 2, 4) == rs.E_INVAL and b"coprime" in lib.e2ers_last_error(h)
    for L, M in ((0, 1), (1, 0), (-2, 1), (rs.MAX_RATIO + 1, 1), (1, rs.MAX_RATIO + 1)):
        assert load(ptr, 65, L, M) == rs.E_INVAL, (L, M)
    long = np.zeros(2 * rs.MAX_PHASE_TAPS + 1, np.float32)
    assert load(long.ctypes.data, long.size, 1, 2) == rs.E_INVAL and b"1024" in lib.e2ers_last_error(h)     # P = 2049
    for bad in (np.nan, np.inf, -np.inf):
        t = taps.copy()
        t[7] = bad
        assert load(t.ctypes.data, t.size, 2, 1) == rs.E_INVAL and b"taps[7]" in lib.e2ers_last_error(h)
    assert lib.e2ers_tile_outputs(h) == 0 and lib.e2ers_tile_outputs(None) == 0

    B, n = 2, 64
    audio = np.zeros((B, n), np.float32)
    wav, lens = np.full((B, 128), 7.0, np.float32), np.zeros(B, np.int64)
    W = C.c_longlong(-7)

    def fwd(nv, a=audio, dtype=rs.F32, stride=n, B=B, n=n):
        arr = None if nv is None else np.asarray(nv, np.int64)   # (kept alive over the call)
        return lib.e2ers_forward(h, None if a is None else a.ctypes.data, dtype, stride, None if arr is None else arr.ctypes.data, B, n,
                                 wav.ctypes.data, None, 128, lens.ctypes.data, C.byref(W))

    assert fwd(None, a=None) == rs.E_INVAL
    assert fwd(None, dtype=2) == rs.E_INVAL and fwd(None, dtype=-1) == rs.E_INVAL
    assert fwd(None, B=0) == rs.E_INVAL and fwd(None, B=rs.MAX_B + 1) == rs.E_INVAL
    assert fwd(None, n=0) == rs.E_INVAL and fwd(None, stride=n - 1) == rs.E_INVAL and fwd(None, n=(1 << 40) + 1, stride=1 << 41) == rs.E_INVAL
    assert fwd([64, 65]) == rs.E_INVAL and b"n_valid[1] = 65" in lib.e2ers_last_error(h)
    assert fwd([-1, 64]) == rs.E_INVAL and b"n_valid[0] = -1" in lib.e2ers_last_error(h)
    odd = np.zeros(2 * n + 1, np.int16)[1:].view(np.uint8)[1:]                                        # an int16 row at an odd address
    assert lib.e2ers_forward(h, odd.ctypes.data, rs.I16, n, None, 1, n, None, None, 0, None, None) == rs.E_INVAL and b"aligned" in lib.e2ers_last_error(h)
    assert fwd(None) == rs.E_STATE and fwd([0, 64]) == rs.E_STATE                                     # valid arguments: call order (nothing loaded)
    assert W.value == -7 and (wav == 7.0).all()
    # the stream: arguments, then call order
    assert lib.e2ers_stream_begin(h, 0, rs.F32) == rs.E_INVAL and lib.e2ers_stream_begin(h, rs.MAX_B + 1, rs.F32) == rs.E_INVAL
    assert lib.e2ers_stream_begin(h, 1, 2) == rs.E_INVAL and lib.e2ers_stream_begin(h, 1, rs.F32) == rs.E_STATE
    nr = C.c_longlong(-7)
    assert lib.e2ers_stream_push(h, audio.ctypes.data, n, -1, 0, C.byref(nr)) == rs.E_INVAL
    assert lib.e2ers_stream_push(h, None, n, 8, 0, C.byref(nr)) == rs.E_INVAL
    assert lib.e2ers_stream_push(h, audio.ctypes.data, 7, 8, 0, C.byref(nr)) == rs.E_INVAL
    assert lib.e2ers_stream_push(h, audio.ctypes.data, n, 8, 0, C.byref(nr)) == rs.E_STATE and nr.value == -7
    assert lib.e2ers_stream_fetch(h, wav.ctypes.data, None, 128, wav.size) == rs.E_STATE
    assert lib.e2ers_profile_read(h, None) == rs.E_INVAL
    assert not lib.e2ers_wav_dev(h) and not lib.e2ers_pcm_dev(h)                                      # nothing resident
    assert lib.e2ers_device_bytes(h) == 0
    assert fwd(None) == rs.E_STATE and lib.e2ers_sync(h) == rs.E_OK                                   # still usable
    lib.e2ers_destroy(h)
    # the Python layer raises ValueError / TypeError for the same, and for what it checks itself
    with pytest.raises(ValueError):
        rs.Resampler(22050, 16000, taps=np.zeros(64, np.float32)).load()
    with pytest.raises(ValueError):
        rs.Resampler(22050, 16000, taps=np.full(65, np.nan, np.float32)).load()
    with pytest.raises(ValueError):
        rs.Resampler(22050, 0)
    r = rs.Resampler(2, 1)
    with pytest.raises(ValueError):
        rs._audio_layout(np.zeros(5, np.float32))
    with pytest.raises(TypeError):
        rs._audio_layout(np.zeros((1, 5), np.float64))
    r.close()
