"""GPU tests (-m gpu) of the resampler's hook-up above the library, on the tiny config: output_rate= of TTS.inference_ids / TTS.inference,
resample= of Synthesizer.synthesis, wav_rate= of UnsupervisedFastSpeech2.align_audio and output_rate= of Denoiser.stream.  The
arithmetic is pinned by tests/test_gpu_resample.py; here the plumbing is: lengths, silence, and that every default is today's result."""
import wave

import numpy as np
import pytest

from conftest import load_golden
import mel_ref as mr
import resample_ref as rr
from aligner_cases import fixture_state
from test_gpu_denoiser_api import write_checkpoints
from e2e_tts_amd import config as cfgmod, resample as rs, synth_weights as sw

pytestmark = pytest.mark.gpu


def test_tts_output_rate_and_synthesizer_resample(tmp_path):
    from e2e_tts_amd.api import TTS, Synthesizer
    cfg = cfgmod.tiny_config()
    stats = cfgmod.DEFAULT_STATS
    ac = sw.make_acoustic_state(cfg, stats, 4, seed=7, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=8)
    apath, vpath = write_checkpoints(tmp_path, cfg, ac, voc)
    g2p = lambda t: [4 + (ord(c) % 127) for c in t]   # noqa: E731
    tts = TTS(apath, vpath, max_len=60, text_to_sequence=g2p)
    sr, hop = tts.sample_rate, tts.hop_length
    assert sr == 22050
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [list(rng.integers(4, 131, n)) for n in (25, 9, 31)]
    plain = tts.inference_ids(seqs, "spk_c")
    # None and the model's own rate are today's array
    np.testing.assert_array_equal(tts.inference_ids(seqs, "spk_c", output_rate=None), plain)
    np.testing.assert_array_equal(tts.inference_ids(seqs, "spk_c", output_rate=sr), plain)
    # the per-utterance PCM of the default call (cut out of the combined array by the utterances' lengths) through a Resampler
    batches, revert = TTS.pack_sequences(seqs, 60)
    lens = []
    for ids, ln in batches:
        _, mel_lens, _ = tts.engine.synthesize(ids, ln, np.array([cfgmod.DEFAULT_SPEAKERS["spk_c"]], np.int64))
        lens.extend(int(m) * hop for m in mel_lens)
    lens = [lens[i] for i in revert.tolist()]
    gap = int(0.5 * sr)
    assert plain.size == sum(lens) + len(lens) * gap
    r = rs.Resampler(sr, 16000)
    want, pos = [], 0
    for n in lens:
        out = r.forward(plain[None, pos:pos + n], want=("pcm",))
        assert out["width"] == rr.n_out(n, 320, 441)
        want += [out["pcm"][0], np.zeros(int(0.5 * 16000), np.int16)]
        pos += n + gap
    got = tts.inference_ids(seqs, "spk_c", output_rate=16000)
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, np.concatenate(want))
    # after the denoiser when one is set; and through the text path
    den = tts.inference_ids(seqs, "spk_c", denoise_strength=0.1)
    den16 = tts.inference_ids(seqs, "spk_c", denoise_strength=0.1, output_rate=16000)
    want, pos = [], 0
    for n in lens:
        want += [r.forward(den[None, pos:pos + n], want=("pcm",))["pcm"][0], np.zeros(8000, np.int16)]
        pos += n + gap
    np.testing.assert_array_equal(den16, np.concatenate(want))
    np.testing.assert_array_equal(tts.inference_ids(seqs, "spk_c"), plain)     # (the engine's strength is back at 0)
    t_plain = tts.inference(["xin chao , viet nam"], "spk_b")
    np.testing.assert_array_equal(tts.inference(["xin chao , viet nam"], "spk_b", output_rate=None), t_plain)
    t48 = tts.inference(["xin chao , viet nam"], "spk_b", output_rate=48000)
    n_utt = t_plain.size - gap
    assert t48.size == rr.n_out(n_utt, 320, 147) + 24000 and not t48[-24000:].any()
    # the service wrapper: sr alone labels the file, resample=True converts
    syn = Synthesizer(apath, vpath, output_dir=str(tmp_path / "out"), max_len=60, text_to_sequence=g2p)
    files = {}
    for name, kw in (("plain", {}), ("label", {"sr": 8000}), ("conv", {"sr": 8000, "resample": True})):
        p = syn.synthesis("xin chao , viet nam", save_filepath=str(tmp_path / "out" / f"{name}.wav"), speaker_id="spk_b", **kw)
        with wave.open(p) as f:
            files[name] = (f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), "<i2"))
    assert files["plain"][0] == 22050 and files["label"][0] == 8000 and files["conv"][0] == 8000
    np.testing.assert_array_equal(files["plain"][1], t_plain)
    np.testing.assert_array_equal(files["label"][1], t_plain)                  # the reference's label-only behaviour
    assert files["conv"][1].size == rr.n_out(n_utt, 160, 441) + int(0.5 * 8000)
    r8 = rs.Resampler(sr, 8000)
    np.testing.assert_array_equal(files["conv"][1][:-4000], r8.forward(t_plain[None, :n_utt], want=("pcm",))["pcm"][0])


def test_align_audio_takes_a_recording_at_another_rate():
    """The fixture's recordings upsampled to 44.1 kHz by the float64 definition, handed to align_audio(wav_rate=44100): the library brings
    them back to 22.05 kHz on the device.  Up and down again is not exact (the filters cut at 0.9 x Nyquist), so the mel is compared first,
    within 4 x the mel error of the same round trip made in float64 on the host; the durations are compared on the rows that passed the
    fixture's robustness screen."""
    import torch
    from e2e_tts_amd import models
    g = load_golden(mr.ALIGN_FIXTURE)
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=3, mode="varied")
    state.update(fixture_state(g))
    m = models.UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0)
    m.load_state_dict(sw.to_torch(state))
    stft = models.TorchSTFT(int(g["n_fft"]), int(g["hop"]), int(g["win_length"]), int(g["n_mel"]), int(g["sr"]), float(g["fmin"]), float(g["fmax"]),
                            device="cuda:0", mel_basis=g["mel_basis"])
    audio, nv, hop = mr.fixture_audio(g), g["n_valid"], int(g["hop"])
    up_taps, down_taps = rs.design(22050, 44100)[0], rs.design(44100, 22050)[0]
    B, n = audio.shape
    up = np.zeros((B, 2 * n), np.float32)
    back64 = np.zeros((B, n))
    for b in range(B):
        up[b, :2 * nv[b]] = rr.resample_f64(audio[b, :nv[b]], up_taps, 2, 1).astype(np.float32)
        back64[b, :nv[b]] = rr.resample_f64(up[b, :2 * nv[b]], down_taps, 1, 2)
    # the round trip's own mel error, in float64
    d64 = mr.dft64(int(g["n_fft"]), int(g["win_length"]))
    mel_rt, _, lens = mr.mel_batch(back64, nv, d64, g["mel_basis"].astype(np.float64), hop, float(g["clip"]), np.float64)
    assert np.array_equal(lens, g["mel_lens"])
    own_mean, own_max = mr.valid_stats(mel_rt, g["mel64"], lens)
    # the device's round trip: Resampler, then the mel library on the resident result (the chain align_audio runs)
    r = rs.Resampler(44100, 22050, device=0)
    out = r.forward(up, n_valid=2 * nv, want=())
    assert np.array_equal(out["n_out"], nv)
    mel_dev = stft.frontend.forward(r.resident()[0], out["n_out"], want=("mel",))["mel"]
    got_mean, got_max = mr.valid_stats(mel_dev, g["mel64"], lens)
    print(f"log-mel after 22.05 -> 44.1 -> 22.05 kHz: float64 round trip mean {own_mean:.3e} max {own_max:.3e}; device mean {got_mean:.3e} max {got_max:.3e}; "
          f"tolerance 4 x the float64 figures")
    assert got_mean <= 4 * own_mean and got_max <= 4 * own_max
    ref = m.align_audio(g["speakers"], g["ids"], g["txt_lens"], audio, nv, stft=stft)
    np.testing.assert_array_equal(m.align_audio(g["speakers"], g["ids"], g["txt_lens"], audio, nv, stft=stft, wav_rate=22050)[2].cpu().numpy(),
                                  ref[2].cpu().numpy())                        # the transform's own rate: today's path
    soft, hard, dur, logprob, energy = m.align_audio(g["speakers"], g["ids"], g["txt_lens"], torch.from_numpy(up).cuda(), 2 * nv, return_energy=True,
                                                     stft=stft, wav_rate=44100)
    T, L = int(g["mel_lens"].max()), g["ids"].shape[1]
    assert soft.shape == (B, 1, T, L) and dur.shape == (B, L) and energy.shape == (B, T)
    assert np.array_equal(hard[:, 0].sum(1).cpu().numpy(), dur.cpu().numpy())
    assert np.array_equal(dur.sum(1).cpu().numpy(), g["mel_lens"].astype(np.float32))     # mel_lens follow from the converted lengths
    keep = g["screened"].astype(bool)
    assert keep.any()
    assert np.array_equal(dur.cpu().numpy()[keep], ref[2].cpu().numpy()[keep])
    with pytest.raises(ValueError):
        m.align_audio(g["speakers"], g["ids"], g["txt_lens"], up, np.array([100, 100, 100]), stft=stft, wav_rate=44100)   # too short to reflect


def test_denoiser_stream_at_another_rate():
    from e2e_tts_amd.models import Denoiser, HifiGan
    gold = load_golden("denoiser")
    cfg = cfgmod.tiny_config()
    v = HifiGan(cfg["models"]["hifigan"], device=0)
    v.load_state_dict(sw.to_torch(sw.make_vocoder_state(cfg, seed=int(gold["c_weight_seed"]))))
    v.eval()
    den = Denoiser(v)
    rng = np.random.Generator(np.random.PCG64(2))
    mel = rng.standard_normal((1, 96, cfg["audio"]["mel"]["channels"])).astype(np.float32)
    chunks = [mel[:, a:a + 32] for a in range(0, 96, 32)]
    whole = np.concatenate(list(den.stream(chunks, strength=0.1)), axis=1)
    r = rs.Resampler(22050, 16000)
    for want_pcm in (False, True):
        got = np.concatenate(list(den.stream(chunks, strength=0.1, output_rate=16000, source_rate=22050, want_pcm=want_pcm)), axis=1)
        np.testing.assert_array_equal(got, r.forward(whole, want=("pcm" if want_pcm else "wav",))["pcm" if want_pcm else "wav"])
    np.testing.assert_array_equal(np.concatenate(list(den.stream(chunks, strength=0.1, output_rate=22050)), axis=1), whole)
