"""mel_tail_kernel alone (-m gpu): through e2emel_debug_tail of the mel library's test build the caller's spectrum goes straight into the tail
kernel, launched by the function e2emel_forward launches it through.  Cases and spectra: tests/mel_tail_cases.py; restatement and rules:
tests/mel_tail_ref.py (energy bit for bit, every clamp decision from the restated sum with clamped elements exactly log_clip, the other
elements within K = 4 ulp of the float64 logarithm of the restated sum, frames past frames[b] exactly 0).

The hook does not use the transform's basis: the handles load an all-zero DFT matrix."""
import time

import numpy as np
import pytest

import mel_tail_cases as mc
import mel_tail_ref as tr
from e2e_tts_amd import mel as mp
from test_gpu_kernels import record

pytestmark = pytest.mark.gpu

_T0 = time.time()
_tally = {}
_tiles = set()


@pytest.mark.parametrize("n_mel", mc.N_MELS)
@pytest.mark.parametrize("n_fft,hop", mc.GEOMS)
def test_tail_alone(n_fft, hop, n_mel):
    """T = tile - 1, tile, tile + 1 with ragged rows (all frames, one frame, T - 1) on one handle per (geometry, n_mel)."""
    bins, tile = n_fft // 2 + 1, mc.TILES[n_fft]
    fe = mp.MelFrontend(n_fft, hop, n_mel, device=0)
    try:
        assert fe.tile_frames == tr.tile_frames(bins) == tile          # which of the four tile sizes this case runs, from the library and restated
        _tiles.add(tile)
        fe.load(np.zeros((2 * bins, n_fft), np.float32), mc.basis_of(n_fft, n_mel), float(mc.CLIP))
        for T in mc.t_values(n_fft):
            spec, frames = mc.spectrum(n_fft, hop, n_mel, T)
            fe.poison_workspace()
            mel, energy = fe.debug_tail(spec, frames)
            ref = mc.reference(n_fft, hop, n_mel, T)
            fails, fig = tr.check_tail(ref, mel, energy)
            t = _tally.setdefault(f"tile {tile}", dict(launches=0, energies=0, energies_differing=0, clamped=0, clamped_differing=0, logs=0, logs_off=0, worst_ulp=0.0))
            t["launches"] += 1
            for k in fig:
                t[k] = max(t[k], fig[k]) if k == "worst_ulp" else t[k] + fig[k]
            assert not fails, (n_fft, n_mel, T, fails)
    finally:
        fe.close()


def test_every_tile_size_ran_and_tally():
    assert _tiles == {16, 8, 4, 2}
    for fam, t in sorted(_tally.items()):
        print(f"[mel tail] {fam}: {t['launches']} launches; energies {t['energies']} ({t['energies_differing']} differing); clamped {t['clamped']} "
              f"({t['clamped_differing']} not log_clip); logarithms {t['logs']} ({t['logs_off']} off), worst {t['worst_ulp']:.3g} ulp of K = {tr.K_ULP}")
        record("mel_tail", kernel=fam, **t)
    record("mel_tail_wall", seconds=time.time() - _T0)
    print(f"[mel tail] wall time {time.time() - _T0:.1f} s")
