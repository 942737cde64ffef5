"""CPU checks of what tests/test_gpu_mel_tail.py relies on (tests/mel_tail_ref.py, tests/mel_tail_cases.py): the restated tile sizes against the
library, tail_f32 against the float64 tail of tests/mel_ref.py's formula on a fixture's spectrum, the constructed values (the clamp's three
neighbours, the zero frame, overflow, subnormal squares, the NaN bin's reach), the shape of the designed bands, every listed mutation through
check_tail, and the hook's refusals (no GPU)."""
import ctypes as C

import numpy as np

from conftest import load_golden
import mel_ref as mr
import mel_tail_cases as mc
import mel_tail_ref as tr
from e2e_tts_amd import mel as mp

f32, f64 = np.float32, np.float64
SMALL = (256, 64, 20)                      # the smallest geometry, 20 mel rows


def test_tile_sizes_and_partial_groups():
    for n_fft, hop in mc.GEOMS:
        bins = n_fft // 2 + 1
        assert mp.MelFrontend(n_fft, hop, 80).tile_frames == tr.tile_frames(bins) == mc.TILES[n_fft]
        assert mc.t_values(n_fft) == [mc.TILES[n_fft] - 1, mc.TILES[n_fft], mc.TILES[n_fft] + 1] and tr.cpad_of(bins) % 32 == 0
    assert sorted(mc.TILES.values()) == [2, 4, 8, 16] and [g[0] // 2 + 1 for g in mc.GEOMS] == [129, 1025, 2049, 4097]
    group = {tile: 4 * 64 // tile for tile in mc.TILES.values()}              # mel rows the four wavefronts take per pass
    assert all(4 % g for g in group.values())                                 # n_mel 4: a partial group at every tile size
    assert all(20 % group[t] and 80 % group[t] for t in (8, 4, 2))            # 20 and 80: at the smaller tiles
    assert all(128 % g == 0 for g in group.values())                          # 128: the full-group control


def test_designed_bands():
    for n_fft, hop in mc.GEOMS:
        bins = n_fft // 2 + 1
        for n_mel in mc.N_MELS:
            w = mc.basis_of(n_fft, n_mel)
            band = tr.band_table(w)
            assert np.array_equal(band, mp.band_table(w)) and w.shape == (n_mel, bins)
            width = band[:, 1] - band[:, 0] + 1
            assert width[0] == 1 and band[0, 0] == mc.clip_bin(bins) and w[0, band[0, 0]] == mc.W_CLIP
            assert (width == bins).any()                                      # the dense band
            lo, hi = np.flatnonzero(band[:, 1] == 4), np.flatnonzero(band[:, 1] == bins - 1)
            per_wave = 64 // mc.TILES[n_fft]
            assert any(a // per_wave == b // per_wave and band[a, 0] == 0 and band[b, 0] >= bins - 5 for a in lo for b in hi)   # opposite ends, one wavefront
            if n_mel >= 20:
                assert list(width[:9]) == list(range(1, 10)) and width[9] == 0           # every remainder of the four-bin unroll; the empty band
                assert (w[11, band[11, 0]:band[11, 1] + 1] == 0).any()                   # explicit zeros inside a band
                tri = band[14:]
                assert np.all(tri[1:, 0] <= tri[:-1, 1])                                 # the triangles overlap


def test_tail_f32_against_the_float64_tail_on_a_fixtures_spectrum():
    """mel_ref's lines -- mag = sqrt((re^2 + im^2) + 1e-9), mel = basis @ mag, log(max(mel, clip)), energy = sqrt(sum mag^2) -- in float64 on the
    float32 spectrum of mel_tiny_b3's first row; the float32 restatement within gamma bars of it (all terms positive)."""
    g = load_golden("mel_tiny_b3")
    n_fft, hop, clip = int(g["n_fft"]), int(g["hop"]), float(g["clip"])
    bins = n_fft // 2 + 1
    x = mr.fixture_audio(g)[0, :int(g["n_valid"][0])]
    fr = mr.frames_of_row(x, n_fft, hop)[:x.size // hop]
    spec = (fr.astype(f64) @ mr.fixture_dft(g, f64).T).astype(f32)
    T = spec.shape[0]
    pad = np.zeros((1, T, tr.cpad_of(bins)), f32)
    pad[0, :, :2 * bins] = spec
    mb = g["mel_basis"]
    ref = tr.tail_f32(pad, [T], T, bins, mb, clip)
    re, im = spec[:, :bins].astype(f64), spec[:, bins:].astype(f64)
    mag = np.sqrt((re * re + im * im) + f64(f32(1e-9)))
    mel64, e64 = mag @ mb.astype(f64).T, np.sqrt((mag * mag).sum(1))
    nnz = int((mb != 0).sum(1).max())
    assert np.all(np.abs(ref["energy"][0] - e64) <= mr.gamma(bins + 8) * e64)
    assert np.all(np.abs(ref["acc"][0] - mel64) <= mr.gamma(nnz + 4) * mel64 + 1e-30)
    near = np.abs(mel64 - clip) <= mr.gamma(nnz + 4) * mel64
    assert np.array_equal(ref["clamped"][0][~near], (mel64 <= clip)[~near])
    mel, energy = tr.outputs_of(ref)
    want = np.log(np.maximum(mel64, clip))
    assert np.all(np.abs(mel[0] - want)[~near] <= mr.gamma(nnz + 4) + 4 * mr.U * np.abs(want[~near]))
    assert not tr.check_tail(ref, mel, energy)[0]


def test_constructed_values():
    for n_fft, hop in mc.GEOMS:
        bins = n_fft // 2 + 1
        for n_mel in (4, 20):
            acc, clamped = mc.clip_row_accs(n_fft, hop, n_mel)
            assert np.array_equal(acc, np.array([np.nextafter(mc.CLIP, f32(0)), mc.CLIP, np.nextafter(mc.CLIP, f32(1))], f32))   # one ulp below, on, one ulp above clip
            assert clamped.tolist() == [True, True, False]
        ref = mc.full_reference(n_fft, hop, 20)
        spec = mc.full_spectrum(n_fft, hop, 20)
        band = tr.band_table(mc.basis_of(n_fft, 20))
        # the zero frame: every magnitude sqrt(1e-9), the energy sqrt(bins 1e-9) up to its roundings
        assert np.all(tr.magnitudes(spec[1, 0, :bins], spec[1, 0, bins:2 * bins]) == np.sqrt(f32(1e-9)))
        assert abs(ref["energy"][1, 0] - np.sqrt(bins * 1e-9)) < 1e-6 * np.sqrt(bins * 1e-9)
        # overflow: infinite magnitudes at bins 5 and 7 -> an infinite energy, +inf in the rows whose band holds them with a weight
        mag = tr.magnitudes(spec[2, 0, :bins], spec[2, 0, bins:2 * bins])
        assert np.isinf(mag[5]) and np.isinf(mag[7]) and np.isfinite(np.delete(mag, [5, 7])).all() and np.isinf(ref["energy"][2, 0])
        holds = (band[:, 0] <= 7) & (band[:, 1] >= 5)
        assert holds.any() and np.all(~np.isfinite(ref["acc"][2, 0][holds])) and np.all(np.isfinite(ref["acc"][2, 0][~holds]))
        # subnormal squares and squares that underflow
        with np.errstate(under="ignore"):
            sq, sq0 = (spec[0, 0, 8:16] * spec[0, 0, 8:16]).astype(f32), (spec[0, 0, bins + 8:bins + 16] ** 2).astype(f32)
        assert np.all((sq > 0) & (sq < f32(1.17549435e-38))) and np.all(sq0 == 0)
        # the NaN bin reaches exactly the rows whose band holds it
        holds = (band[:, 0] <= 2) & (band[:, 1] >= 2)
        assert holds.any() and not holds.all() and np.array_equal(np.isnan(ref["acc"][2, 1]), holds) and np.isnan(ref["energy"][2, 1])
        assert ref["clamped"].any() and (~ref["clamped"] & np.isfinite(ref["acc"])).any()       # both sides of the clamp occur
    # the three frames of the clip row exist in every T = tile + 1 launch, and the ragged rows are (T, 1, T - 1)
    assert all(mc.TILES[n] + 1 >= 3 for n in mc.TILES) and mc.frames_of(17) == [17, 1, 16] and mc.frames_of(1) == [1, 1, 1]
    spec, frames = mc.spectrum(256, 64, 20, 15)
    assert spec.shape == (3, 15 + 3, tr.cpad_of(129)) and np.isnan(spec[:, 15:]).all() and np.isnan(spec[:, :, 258:]).all()


# ---------------------------------------------------------------- mutations, through the GPU test's own check function
def _fails(mut, T=17, geom=SMALL):
    n_fft, hop, n_mel = geom
    ref = mc.reference(n_fft, hop, n_mel, T)
    mel, energy = tr.outputs_of(mc.reference(n_fft, hop, n_mel, T, mut))
    return tr.check_tail(ref, mel, energy)[0]


def test_the_restatement_passes_its_own_check():
    for T in mc.t_values(256):
        assert not _fails(None, T)


def test_mutations_of_the_magnitude_and_the_energy():
    assert _fails("eps_outside") and _fails("fused_squares")
    assert any("energies" in f for f in _fails("ascending"))


def test_mutations_of_the_band_and_the_frames():
    assert _fails("drop_last_bin") and _fails("skip_last_frame") and _fails("skip_last_frame", T=15) and _fails("skip_last_frame", T=16)
    # the band widened by one adds fmaf(0, mag, acc): nothing on finite magnitudes, a NaN where the neighbour's magnitude is infinite
    # (row 12's band ends at bin 4, the spectra put an infinity at bin 5)
    assert _fails("band_wide")
    n_fft, hop, n_mel = SMALL
    a, b = mc.full_reference(n_fft, hop, n_mel), mc.full_reference(n_fft, hop, n_mel, "band_wide")
    fin = np.isfinite(b["acc"])
    assert np.array_equal(a["acc"][fin], b["acc"][fin]) and (~fin & np.isfinite(a["acc"])).any()


def test_lt_for_le_at_the_clamp_cannot_be_caught():
    """`acc < clip` differs from `acc <= clip` on the one element whose sum is exactly clip, where it writes logf(clip) instead of log_clip; a
    logf within K ulp may return the very same float (a correctly rounded one does: log_clip IS the float64 logarithm rounded once), so the
    rules cannot tell the two apart.  Asserted as such; the element is still in the cases, for a logf that does not."""
    n_fft, hop, n_mel = SMALL
    a, b = mc.full_reference(n_fft, hop, n_mel), mc.full_reference(n_fft, hop, n_mel, "lt_clamp")
    changed = a["clamped"] != b["clamped"]
    assert changed.sum() == 1 and a["acc"][changed][0] == mc.CLIP
    assert f32(np.log(f64(mc.CLIP))) == a["log_clip"] and not _fails("lt_clamp")


def test_hook_refusals_without_a_gpu():
    lib = mp.load_library()
    assert hasattr(lib, "e2emel_debug_tail"), "the tests load the test build of the mel library"
    h = C.c_void_p()
    assert lib.e2emel_create(0, 256, 64, 20, C.byref(h)) == mp.E_OK
    spec, fr = np.zeros((2, 5 + 3, tr.cpad_of(129)), f32), np.array([5, 1], np.int32)
    mel, en = np.zeros((2, 5, 20), f32), np.zeros((2, 5), f32)

    def call(s=spec, f=fr, B=2, T=5, hh=h):
        return lib.e2emel_debug_tail(hh, None if s is None else s.ctypes.data, None if f is None else f.ctypes.data, B, T, mel.ctypes.data, en.ctypes.data)

    assert call(hh=None) == mp.E_INVAL and call(s=None) == mp.E_INVAL and call(f=None) == mp.E_INVAL
    assert call(B=0) == mp.E_INVAL and call(B=mp.MAX_B + 1) == mp.E_INVAL and call(T=0) == mp.E_INVAL and call(T=(1 << 20) + 1) == mp.E_INVAL
    assert call(f=np.array([6, 1], np.int32)) == mp.E_INVAL and call(f=np.array([5, -1], np.int32)) == mp.E_INVAL
    assert b"frames[b]" in lib.e2emel_last_error(h)
    assert call() == mp.E_STATE and not mel.any() and lib.e2emel_device_bytes(h) == 0      # valid arguments, nothing loaded: nothing opened
    lib.e2emel_destroy(h)
