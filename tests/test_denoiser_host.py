"""Host checks (-m "not gpu") of the vocoder-bias denoiser's restatement and Python mirror against tests/golden/denoiser.npz, which
tools/make_denoiser_goldens.py wrote from the reference's own module (V/denoiser.py) run row by row.

  * tests/denoiser_ref.py in float64 IS the reference's float64 run (<= 1e-12), so it may stand in for it on shapes no fixture has;
  * the same in float32 in the 4-tap row form the engine computes (two "same" convolutions over rows of `hop` samples) lies as close to
    the float64 run as the reference's own fp32 run does -- the bars of tests/test_gpu_denoiser.py (4 x mean, 8 x max) hold for it here;
  * e2e_tts_amd.denoiser.stft_bases gives the reference's buffers bit for bit;
  * strength 0 reconstructs the input; bad geometries and lengths are refused with ValueError.
"""
import numpy as np
import pytest

from conftest import load_golden
import denoiser_ref as dr
from e2e_tts_amd import denoiser as dn

CASES = ("a", "b")


@pytest.fixture(scope="module")
def gold():
    return load_golden("denoiser")


@pytest.fixture(scope="module")
def bases(gold):
    out = {}
    for tag in CASES:
        N, V = (int(x) for x in gold[f"{tag}_geometry"])
        out[tag] = (N, N // V) + dn.stft_bases(N, N // V, N)
    return out


def valid_dist(a, b, n_valid):
    d = np.concatenate([np.abs(a[i, :nb].astype(np.float64) - b[i, :nb].astype(np.float64)) for i, nb in enumerate(n_valid)])
    return float(d.mean()), float(d.max())


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("si", (0, 1))
def test_float64_restatement_is_the_references_float64_run(gold, bases, tag, si):
    N, hop, fwd, inv, win_sq = bases[tag]
    nv, s = gold[f"{tag}_n_valid"], float(gold[f"{tag}_strengths"][si])
    got = dr.denoise_batch(dr.denoise_frames, gold[f"{tag}_audio"], nv, gold[f"{tag}_bias"], s, fwd, inv, win_sq, hop, dtype=np.float64)
    mean, mx = valid_dist(got, gold[f"{tag}_out64_s{si}"], nv)
    print(f"{tag} strength {s}: float64 restatement vs reference float64: mean {mean:.2e} max {mx:.2e}")
    assert mx <= 1e-12
    for b, nb in enumerate(nv):
        assert not got[b, nb:].any()


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("si", (0, 1))
def test_float32_row_form_is_as_close_as_the_references_fp32(gold, bases, tag, si):
    N, hop, fwd, inv, win_sq = bases[tag]
    nv, s = gold[f"{tag}_n_valid"], float(gold[f"{tag}_strengths"][si])
    got = dr.denoise_batch(dr.denoise_rows, gold[f"{tag}_audio"], nv, gold[f"{tag}_bias"], s, fwd, inv, win_sq, hop)
    assert got.dtype == np.float32
    mean, mx = valid_dist(got, gold[f"{tag}_out64_s{si}"], nv)
    dref, dmax = float(gold[f"{tag}_dref"][si]), float(gold[f"{tag}_dmax"][si])
    print(f"{tag} strength {s}: 4-tap float32 vs reference float64: mean {mean:.3e} (reference fp32: {dref:.3e}) max {mx:.3e} ({dmax:.3e})")
    assert mean <= 4 * dref and mx <= 8 * dmax
    # the fixture's own claims: the fp32 output is dref from the float64 one, and the effect dwarfs it
    m2, x2 = valid_dist(gold[f"{tag}_out32_s{si}"], gold[f"{tag}_out64_s{si}"], nv)
    assert m2 == pytest.approx(dref, rel=1e-9) and x2 == pytest.approx(dmax, rel=1e-9)
    if s > 0:
        assert float(gold[f"{tag}_effect"][si]) >= 100 * dref


def test_stft_bases_are_the_references_buffers(gold):
    fwd, inv, win_sq = dn.stft_bases(1024, 256, 1024)
    assert fwd.shape == inv.shape == (1026, 1024) and fwd.dtype == inv.dtype == np.float32 and win_sq.dtype == np.float64
    rows = gold["d_rows"]
    np.testing.assert_array_equal(rows, np.arange(0, 1026, 37))
    np.testing.assert_array_equal(fwd[rows], gold["d_fwd_rows"])
    np.testing.assert_array_equal(inv[rows], gold["d_inv_rows"])
    assert np.abs(fwd.astype(np.float64)).sum() == pytest.approx(float(gold["d_fwd_l1"]), rel=1e-12)
    assert np.abs(inv.astype(np.float64)).sum() == pytest.approx(float(gold["d_inv_l1"]), rel=1e-12)
    # periodic Hann, squared; at 4-fold overlap its sum over the hops is the constant 1.5
    k = np.arange(1024)
    np.testing.assert_allclose(win_sq, (0.5 - 0.5 * np.cos(2 * np.pi * k / 1024)) ** 2, atol=1e-15)
    np.testing.assert_allclose(win_sq.reshape(4, 256).sum(0), 1.5, atol=1e-12)
    assert dn.engine_window(win_sq, 1024, 1024, "hann") is None


def test_short_window_is_centre_padded():
    fwd, inv, win_sq = dn.stft_bases(512, 128, 256)
    assert not win_sq[:128].any() and not win_sq[384:].any() and win_sq[129:384].all()
    assert not fwd[:, :128].any() and not inv[:, 384:].any()
    w = dn.engine_window(win_sq, 512, 256, "hann")
    assert w is not None and w.dtype == np.float32 and w.shape == (512,)
    with pytest.raises(ValueError):
        dn.stft_bases(512, 128, 1024)


def test_envelope_minimum_over_the_kept_range():
    """What lets the kernel divide wherever the envelope exceeds FLT_MIN: over the samples that are kept it is far from it."""
    for N, V in ((1024, 4), (512, 2), (1024, 8)):
        hop = N // V
        win_sq = dn.stft_bases(N, hop, N)[2]
        for F in (N // 2 // hop + 2, 9):
            env = dr.envelope(win_sq, F, hop)[N // 2:N // 2 + (F - 1) * hop]
            assert env.min() > (0.4 if V == 2 else 1.2), (N, V, F, env.min())   # Hann^2 at 2-fold overlap dips to 0.5, 4-fold is 1.5, 8-fold 3


@pytest.mark.parametrize("tag", CASES)
def test_strength_zero_reconstructs_the_input(gold, bases, tag):
    N, hop, fwd, inv, win_sq = bases[tag]
    nv, audio = gold[f"{tag}_n_valid"], gold[f"{tag}_audio"]
    # the yardstick is the reference's own reconstruction (its strength-0 output against its input: the float32 bases are an inverse pair
    # to float32 accuracy only); a float32 restatement in another summation order gets the factors of the GPU test
    ref_mean, ref_max = valid_dist(gold[f"{tag}_out32_s1"], audio, nv)
    assert float(gold[f"{tag}_strengths"][1]) == 0.0 and ref_max < 1e-6
    for fn, kw in ((dr.denoise_frames, dict(dtype=np.float64)), (dr.denoise_rows, {})):
        got = dr.denoise_batch(fn, audio, nv, gold[f"{tag}_bias"], 0.0, fwd, inv, win_sq, hop, **kw)
        mean, mx = valid_dist(got, audio, nv)
        print(f"{tag} {fn.__name__}: strength 0 vs input mean {mean:.3e} max {mx:.3e} (reference: {ref_mean:.3e} / {ref_max:.3e})")
        assert mean <= 4 * ref_mean and mx <= 8 * ref_max


def test_rows_at_or_under_half_a_filter_pass_through(gold, bases):
    N, hop, fwd, inv, win_sq = bases["a"]
    audio = gold["a_audio"][:2, :1024].copy()
    got = dr.denoise_batch(dr.denoise_rows, audio, [512, 256], gold["a_bias"], 0.1, fwd, inv, win_sq, hop)
    np.testing.assert_array_equal(got[0, :512], audio[0, :512])
    np.testing.assert_array_equal(got[1, :256], audio[1, :256])
    assert not got[0, 512:].any() and not got[1, 256:].any()
    with pytest.raises(ValueError):
        dr.denoise_rows(audio[0, :512], gold["a_bias"], 0.1, fwd, inv, win_sq, hop)


@pytest.mark.parametrize("N,hop", [(1024, 1024), (1024, 64), (1000, 250), (1024, 300), (96, 24), (4096, 2048), (0, 0), (1024, 0)])
def test_mirror_refuses_unserved_geometries(N, hop):
    with pytest.raises(ValueError):
        dn.check_geometry(N, hop)
    with pytest.raises(ValueError):
        dn.stft_bases(N, hop, N)


def test_mirror_accepts_served_geometries():
    assert [dn.check_geometry(N, h) for N, h in ((1024, 256), (512, 256), (1024, 128), (2048, 1024), (64, 32))] == [4, 2, 8, 2, 2]


def test_mirror_refuses_lengths_that_are_no_multiple_of_the_hop():
    np.testing.assert_array_equal(dn.check_lengths([4096, 0, 768], 4096, 256), [4096, 0, 768])
    for bad in ([4096, 100], [4352], [-256], [255]):
        with pytest.raises(ValueError):
            dn.check_lengths(bad, 4096, 256)
