"""GPU tests (-m gpu) of the mel front-end on the HIP path (include/e2etts_mel.h, e2e_tts_amd/mel.py, models.TorchSTFT / generate_melspecs /
UnsupervisedFastSpeech2.align_audio) against the reference's fixtures (tools/make_mel_goldens.py).

Bars (tests/mel_ref.py, against the reference in float64): every element within its derived bar, the mean error within 4 x the reference's
own mean |fp32 - float64| on the same fixture.  What is claimed to be exact is compared bit for bit: frames past mel_lens (zeros), the zero
stretch (log 1e-5 in fp32), a row alone against the same row in a batch, int16 against fp32 input, a dense basis against its banded form.

Measured on an MI355X -- see profiles/mel/README.md."""
import numpy as np
import pytest

from conftest import load_golden
import mel_ref as mr
from aligner_cases import fixture_state
from e2e_tts_amd import mel as mp

pytestmark = pytest.mark.gpu

ALL = mr.FIXTURES + [mr.ALIGN_FIXTURE]
_HANDLES, _RUNS = {}, {}
LOG_CLIP = np.log(np.float32(1e-5))


def frontend(n_fft, hop, n_mel, basis, win=None, tag=""):
    """One handle per (geometry, basis), loaded once."""
    key = (n_fft, hop, n_mel, win, tag, basis.tobytes())
    if key not in _HANDLES:
        fe = mp.MelFrontend(n_fft, hop, n_mel, device=0)
        fe.load(mp.dft_basis(n_fft, win), basis, 1e-5)
        _HANDLES[key] = fe
    return _HANDLES[key]


def frontend_of(g):
    return frontend(int(g["n_fft"]), int(g["hop"]), int(g["n_mel"]), g["mel_basis"], int(g["win_length"]))


def run_fixture(name):
    """One e2emel_forward per fixture (host fp32 samples in, every output out), shared by the tests below and left unchanged."""
    if name not in _RUNS:
        g = load_golden(name)
        fe = frontend_of(g)
        r = fe.forward(mr.fixture_audio(g), g["n_valid"])
        _RUNS[name] = (g, fe, r)
    return _RUNS[name]


def tiny_signal(B, n, seed=0):
    """[B, n] samples on the int16 grid: a sine plus noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)[None, :]
    x = 0.5 * np.sin(0.07 * (1 + np.arange(B))[:, None] * t) + 0.1 * rng.standard_normal((B, n))
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("name", ALL)
def test_fixture_within_the_bars_of_the_float64_reference(name):
    g, fe, r = run_fixture(name)
    assert r["T"] == int(g["mel_lens"].max()) == r["mel"].shape[1] and np.array_equal(r["mel_lens"], g["mel_lens"]) and r["mel_lens"].dtype == np.int64
    assert mr.check_against_fixture(r["mel"], r["energy"], g, label=f"{name} HIP") == []   # includes: exactly 0 past mel_lens
    assert np.isfinite(r["mel"]).all() and np.isfinite(r["energy"]).all()


@pytest.mark.parametrize("name", mr.FIXTURES)
def test_the_zero_stretch_is_exactly_log_clip(name):
    g, fe, r = run_fixture(name)
    assert len(g["zero_frames"])
    for b, f0, f1 in g["zero_frames"]:
        assert (r["mel"][b, f0:f1] == LOG_CLIP).all()
        assert (r["energy"][b, f0:f1] == r["energy"][b, f0]).all() and abs(r["energy"][b, f0] - np.sqrt((int(g["n_fft"]) // 2 + 1) * 1e-9)) < 1e-7


@pytest.mark.parametrize("name", ["mel_tiny_b3", "mel_full_b2"])
def test_a_row_alone_equals_its_row_of_the_batch(name):
    g, fe, r = run_fixture(name)
    audio = mr.fixture_audio(g)
    for b, nv in enumerate(g["n_valid"]):
        fe.poison_workspace()
        one = fe.forward(np.ascontiguousarray(audio[b:b + 1, :nv]))           # B = 1, n = the row's own length, n_valid NULL
        t = int(g["mel_lens"][b])
        assert one["T"] == t
        assert np.array_equal(one["mel"][0], r["mel"][b, :t]) and np.array_equal(one["energy"][0], r["energy"][b, :t])
    # the poisoned workspace changes nothing, on the batch either; nor does a larger call in between (workspaces only grow)
    fe.poison_workspace()
    again = fe.forward(audio, g["n_valid"])
    assert np.array_equal(again["mel"], r["mel"]) and np.array_equal(again["energy"], r["energy"])
    before = fe.device_bytes()
    fe.forward(audio[:1], g["n_valid"][:1])
    assert fe.device_bytes() == before


@pytest.mark.parametrize("name", ["mel_tiny_b3", "mel_48k_b1"])
def test_int16_input_equals_fp32_input(name):
    import torch
    g, fe, r = run_fixture(name)
    pcm = fe.forward(g["pcm"], g["n_valid"])
    assert np.array_equal(pcm["mel"], r["mel"]) and np.array_equal(pcm["energy"], r["energy"])
    # samples resident in HBM, rows strided (a view of a wider buffer), both types
    wide = torch.zeros((g["pcm"].shape[0], g["pcm"].shape[1] + 13), dtype=torch.int16, device="cuda")
    wide[:, :g["pcm"].shape[1]] = torch.from_numpy(g["pcm"])
    dev = fe.forward(wide[:, :g["pcm"].shape[1]], g["n_valid"])
    assert np.array_equal(dev["mel"], r["mel"]) and np.array_equal(dev["energy"], r["energy"])
    devf = fe.forward(torch.from_numpy(mr.fixture_audio(g)).cuda(), g["n_valid"])
    assert np.array_equal(devf["mel"], r["mel"]) and np.array_equal(devf["energy"], r["energy"])


def test_tile_edges_of_the_fused_kernel():
    """T = tile - 1, tile, tile + 1 frames and a ragged batch whose shortest row has one frame, tiny geometry; against the float32 restatement
    under the derived per-element bars of tests/mel_ref.py."""
    g = load_golden("mel_tiny_b3")
    fe = frontend_of(g)
    n_fft, hop, tile = int(g["n_fft"]), int(g["hop"]), fe.tile_frames
    assert tile == 16
    pcm = tiny_signal(3, (2 * tile + 3) * hop + 7, seed=4)
    audio = pcm.astype(np.float32) / np.float32(32768.0)
    d64, mb64 = mr.dft64(n_fft), g["mel_basis"].astype(np.float64)
    cases = [np.array([t * hop]) for t in (tile - 1, tile, tile + 1)] + [np.array([(2 * tile + 3) * hop + 7, hop + 18, tile * hop + 31])]   # hop + 18 = 50 samples: one frame, just past (n_fft - hop) / 2 = 48
    for nv in cases:
        B = len(nv)
        r = fe.forward(np.ascontiguousarray(audio[:B, :nv.max()]), nv)
        ref = mr.mel_batch(audio[:B].astype(np.float64), nv, d64, mb64, hop, dtype=np.float64)
        lens = nv // hop
        assert np.array_equal(r["mel_lens"], lens) and r["T"] == lens.max()
        bar_mel, bar_e = mr.derived_bars(audio[:B], nv, g)
        for b, t in enumerate(lens):
            assert (np.abs(r["mel"][b, :t] - ref[0][b, :t]) <= bar_mel[b, :t]).all() and (np.abs(r["energy"][b, :t] - ref[1][b, :t]) <= bar_e[b, :t]).all()
            assert not r["mel"][b, t:].any() and not r["energy"][b, t:].any()
        em = mr.valid_stats(r["mel"], ref[0], lens)[0]
        print(f"frames {lens.tolist()}: mel mean |err| {em:.3e}")   # (no aggregate bar: the reference's own error is known on the fixtures only)


def test_dense_walk_equals_the_banded_walk():
    """The same matrix summed over its recorded bands and, with the test build's hook, as the degenerate band [0, bins - 1] of every row
    (what a dense caller-supplied matrix is): the explicit zeros outside the bands add exact zeros, so the bits are the same.  The dense
    fixture's matrix records the degenerate band by itself."""
    for name in ("mel_tiny_b3", "mel_full_b2"):
        g, fe, r = run_fixture(name)
        audio = mr.fixture_audio(g)
        fe.force_dense(True)
        try:
            dense = fe.forward(audio, g["n_valid"])
        finally:
            fe.force_dense(False)
        assert np.array_equal(dense["mel"], r["mel"]) and np.array_equal(dense["energy"], r["energy"])
        back = fe.forward(audio, g["n_valid"])
        assert np.array_equal(back["mel"], r["mel"])
    gd = load_golden("mel_tiny_dense_b2")
    assert (mp.band_table(gd["mel_basis"]) == [0, gd["mel_basis"].shape[1] - 1]).all()
    # an interior zero inside a band is walked over and changes no other row; an all-zero row is the empty band: log(clip)
    g, fe, r = run_fixture("mel_tiny_b3")
    holes = g["mel_basis"].copy()
    band = mp.band_table(holes)
    for m, (a, b) in enumerate(band[:-1]):
        if b - a >= 2:
            holes[m, (a + b) // 2] = 0
    holes[-1] = 0
    assert np.array_equal(mp.band_table(holes)[:-1], band[:-1])
    h = frontend(int(g["n_fft"]), int(g["hop"]), int(g["n_mel"]), holes, tag="holes").forward(mr.fixture_audio(g), g["n_valid"])
    untouched = [m for m, (a, b) in enumerate(band[:-1]) if b - a < 2]
    assert np.array_equal(h["mel"][:, :, untouched], r["mel"][:, :, untouched]) and np.array_equal(h["energy"], r["energy"])
    for b, t in enumerate(g["mel_lens"]):
        assert (h["mel"][b, :t, -1] == LOG_CLIP).all()


def test_mirror_shapes_devices_and_function_form():
    import torch
    from e2e_tts_amd import models
    g, fe, r = run_fixture("mel_full_b2")
    stft = models.TorchSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0, device="cuda:0")
    assert stft.mel_basis.shape == (80, 513) and stft.mel_basis.is_cuda and stft.window.shape == (1024,) and stft.window.is_cuda
    assert np.array_equal(stft.mel_basis.cpu().numpy(), g["mel_basis"]) and stft.stft_pad == (384, 384)
    audio = mr.fixture_audio(g)
    n = int(g["n_valid"].min())
    x = torch.from_numpy(np.ascontiguousarray(audio[:, :n]))
    mel, energy = stft.mel_spectrogram(x, return_energy=True)
    T = n // 256
    assert mel.shape == (2, 80, T) and energy.shape == (2, T) and mel.is_cuda and energy.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous()
    only = stft.mel_spectrogram(x.cuda())
    assert isinstance(only, torch.Tensor) and torch.equal(only, mel)
    # every row of a rectangular batch is the row alone: row 0 is the fixture's row 0 cut to n samples
    one = fe.forward(np.ascontiguousarray(audio[:1, :n]))
    assert np.array_equal(mel[0].T.cpu().numpy(), one["mel"][0]) and np.array_equal(energy[0].cpu().numpy(), one["energy"][0])
    ragged, e2 = stft.mel_spectrogram(torch.from_numpy(audio), return_energy=True, n_valid=g["n_valid"])
    assert np.array_equal(ragged.transpose(1, 2).cpu().numpy(), r["mel"]) and np.array_equal(e2.cpu().numpy(), r["energy"])
    fn = models.generate_melspecs(x, 1024, 80, 22050, 256, 1024, 0.0, 8000.0)
    assert torch.equal(fn, mel)
    with pytest.raises(NotImplementedError, match="stft.py:46"):
        stft.mel_spectrogram(x, center=True)
    with pytest.raises(NotImplementedError):
        models.generate_melspecs(x, center=True)
    with pytest.raises(AssertionError):
        stft.mel_spectrogram(x * 3.0)
    with pytest.raises(ValueError):
        stft.mel_spectrogram(x[:, :300])            # 300 <= (n_fft - hop) / 2: cannot be reflected


def test_align_audio_gives_the_references_durations():
    """Recording -> mel -> durations on the device, against the reference's chain (its mel_spectrogram, AlignmentEncoder and b_mas on the CPU)
    on the rows whose durations survived the fixture's screen (mel perturbed by 10 x its derived bar), and against align() on the
    reference's mel."""
    import torch
    from e2e_tts_amd import config as cfgmod, models, synth_weights as sw
    g = load_golden(mr.ALIGN_FIXTURE)
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    assert fs["encoder_hidden"] == int(g["hidden"])
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=3, mode="varied")
    state.update(fixture_state(g))                # the fixture's aligner, phoneme and speaker tables
    m = models.UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0)
    m.load_state_dict(sw.to_torch(state))
    stft = models.TorchSTFT(int(g["n_fft"]), int(g["hop"]), int(g["win_length"]), int(g["n_mel"]), int(g["sr"]), float(g["fmin"]), float(g["fmax"]),
                            device="cuda:0", mel_basis=g["mel_basis"])
    keep = g["screened"].astype(bool)
    assert keep.any() and g["screen"][0] == 10.0
    soft, hard, dur, logprob, energy = m.align_audio(g["speakers"], g["ids"], g["txt_lens"], g["pcm"], g["n_valid"], return_energy=True, stft=stft)
    B, L, T = g["ids"].shape[0], g["ids"].shape[1], int(g["mel_lens"].max())
    assert soft.shape == hard.shape == logprob.shape == (B, 1, T, L) and dur.shape == (B, L) and energy.shape == (B, T) and dur.is_cuda and energy.is_cuda
    assert np.array_equal(dur.cpu().numpy()[keep], g["dur"][keep])
    assert np.array_equal(hard[:, 0].sum(1).cpu().numpy(), dur.cpu().numpy())
    _, fe, r = run_fixture(mr.ALIGN_FIXTURE)
    assert np.array_equal(energy.cpu().numpy(), r["energy"])
    via_mel = m.align(g["speakers"], g["ids"], g["txt_lens"], g["mel32"], g["mel_lens"])
    assert np.array_equal(via_mel[2].cpu().numpy()[keep], dur.cpu().numpy()[keep])
    fp32 = m.align_audio(g["speakers"], g["ids"], g["txt_lens"], torch.from_numpy(mr.fixture_audio(g)).cuda(), g["n_valid"], stft=stft)
    assert len(fp32) == 4 and torch.equal(fp32[2], dur) and torch.equal(fp32[0], soft)
    with pytest.raises(ValueError):
        m.align_audio(g["speakers"], g["ids"], g["txt_lens"], g["pcm"], np.array([100, 100, 100]), stft=stft)
    # without stft=: the transform of the model's own audio configuration (the shipped defaults are the fixture's geometry)
    au = cfgmod.default_config()["audio"]
    assert (au["stft"]["filter_length"], au["stft"]["hop_length"], au["stft"]["win_length"], au["signal"]["sampling_rate"], au["mel"]["mel_fmin"],
            au["mel"]["mel_fmax"]) == (int(g["n_fft"]), int(g["hop"]), int(g["win_length"]), int(g["sr"]), float(g["fmin"]), float(g["fmax"]))
    own = m.align_audio(g["speakers"], g["ids"], g["txt_lens"], g["pcm"], g["n_valid"])
    assert np.array_equal(m._stft.mel_basis.cpu().numpy(), g["mel_basis"]) and torch.equal(own[2], dur) and torch.equal(own[0], soft)
    # a model of another rate has no known transform until it is told one
    m16 = models.UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0, sampling_rate=16000)
    with pytest.raises(ValueError, match="set_audio_config"):
        m16.align_audio(g["speakers"], g["ids"], g["txt_lens"], g["pcm"], g["n_valid"])
    m16.set_audio_config({"stft": {"filter_length": 512, "hop_length": 256, "win_length": 512}, "mel": {"channels": int(g["n_mel"]), "mel_fmin": 50.0, "mel_fmax": None},
                          "signal": {"sampling_rate": 16000}})
    s16 = m16._default_stft()
    assert (s16.filter_length, s16.hop_length, s16.sampling_rate, s16.fmin, s16.fmax) == (512, 256, 16000, 50.0, None)
    assert np.array_equal(s16.mel_basis.cpu().numpy(), mp.mel_filterbank(16000, 512, int(g["n_mel"]), 50.0, None))


def test_a_wavefront_of_empty_bands_walks_nothing():
    """An all-zero basis, and a basis whose last aligned group of 64 / tile = 4 rows is zero (masked top channels) while the others are not:
    a wavefront whose rows all have the empty band reads nothing and writes log(clip); the other rows keep their bits."""
    g, fe, r = run_fixture("mel_tiny_b3")
    audio, M = mr.fixture_audio(g), int(g["n_mel"])
    assert 64 // fe.tile_frames == 4 and M % 4 == 0
    zero = frontend(int(g["n_fft"]), int(g["hop"]), M, np.zeros_like(g["mel_basis"]), tag="zero").forward(audio, g["n_valid"])
    masked_basis = g["mel_basis"].copy()
    masked_basis[M - 4:] = 0
    masked = frontend(int(g["n_fft"]), int(g["hop"]), M, masked_basis, tag="masked").forward(audio, g["n_valid"])
    assert np.array_equal(zero["energy"], r["energy"]) and np.array_equal(masked["energy"], r["energy"])
    assert np.array_equal(masked["mel"][:, :, :M - 4], r["mel"][:, :, :M - 4])
    for b, t in enumerate(g["mel_lens"]):
        assert (zero["mel"][b, :t] == LOG_CLIP).all() and (masked["mel"][b, :t, M - 4:] == LOG_CLIP).all()
        assert not zero["mel"][b, t:].any() and not masked["mel"][b, t:].any()
