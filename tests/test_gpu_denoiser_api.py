"""GPU tests (-m gpu) of the denoiser's Python surface above Engine, on the tiny config: models.Denoiser (the reference's class:
constructor, bias_spec, forward), and denoise_strength= of TTS.inference_ids / TTS.inference / Synthesizer.synthesis.  The arithmetic
is pinned by tests/test_gpu_denoiser.py; here the plumbing is: shapes, devices, first-use calibration, recalibration after other
weights, and that the engine's strength is back at 0 after a denoised call."""
import json
import wave

import numpy as np
import pytest

from conftest import load_golden
from e2e_tts_amd import config as cfgmod, denoiser as dn, synth_weights as sw

pytestmark = pytest.mark.gpu


def write_checkpoints(tmp_path, cfg, ac, voc):
    import torch
    import yaml
    d, v = tmp_path / "exps" / "acoustic", tmp_path / "exps" / "vocoder"
    d.mkdir(parents=True)
    v.mkdir(parents=True)
    torch.save({"state_dict": sw.to_torch(ac), "optimizer": {}}, d / "statedict.pt")
    torch.save({"state_dict": sw.to_torch(voc)}, v / "statedict.pt")
    full = dict(cfg)
    full["train"] = {"seed": 1234}
    yaml.safe_dump(full, open(d / "config.yaml", "w"))
    json.dump(cfgmod.DEFAULT_SPEAKERS, open(d / "speakers.json", "w"))
    json.dump(cfgmod.DEFAULT_STATS, open(d / "stats.json", "w"))
    return str(d / "statedict.pt"), str(v / "statedict.pt")


def test_models_denoiser_mirrors_the_references_class():
    import torch
    from e2e_tts_amd.models import Denoiser, HifiGan
    gold = load_golden("denoiser")
    cfg = cfgmod.tiny_config()
    v = HifiGan(cfg["models"]["hifigan"], device=0)
    v.load_state_dict(sw.to_torch(sw.make_vocoder_state(cfg, seed=int(gold["c_weight_seed"]))))
    v.eval()
    den = Denoiser(v)   # the reference's defaults: (1024, 4), win_length 1024, mode='zeros'
    assert den.filter_length == 1024 and den.hop_length == 256
    assert tuple(den.bias_spec.shape) == (1, 513, 1) and den.bias_spec.is_cuda and den.bias_spec.dtype == torch.float32
    ref = gold["c_bias_spec"].astype(np.float64)
    rel = float(np.abs(den.bias_spec[0, :, 0].cpu().numpy() - ref).sum() / np.abs(ref).sum())
    assert rel <= 1e-4, rel   # the bar of test_gpu_denoiser.py's calibration test
    audio = v(torch.from_numpy(gold["c_mel"]))   # [2, 1, 2560] on the GPU, as the reference hands it on
    out = den(audio.squeeze(1), strength=float(gold["c_strength"]))
    assert tuple(out.shape) == (2, 1, 2560) and out.is_cuda and out.dtype == torch.float32
    d = np.abs(out[:, 0].cpu().numpy().astype(np.float64) - gold["c_out64"])
    assert d.mean() <= 1e-6   # the fixture's audio and bias to 1e-7: the plumbing carries the engine's result (bars: test_gpu_denoiser.py)
    # per-row lengths, numpy input, default strength
    x = audio.squeeze(1).cpu().numpy()
    o2 = den(x, n_valid=[2560, 1280])
    assert tuple(o2.shape) == (2, 1, 2560) and not o2[1, 0, 1280:].any()
    np.testing.assert_array_equal(o2[1, 0, :1280].cpu().numpy(), den(x[1:, :1280])[0, 0].cpu().numpy())
    with pytest.raises(ValueError):
        den(x[:, :2500])          # not a multiple of the hop
    with pytest.raises(ValueError):
        den(x[0])                 # [n], not [B, n]
    # mode='normal': a random mel instead of zeros, another bias; other geometry
    torch.manual_seed(5)
    den2 = Denoiser(v, filter_length=512, n_overlap=2, win_length=512, mode="normal")
    assert tuple(den2.bias_spec.shape) == (1, 257, 1) and den2.hop_length == 256
    assert float(den2.bias_spec.abs().sum()) > 0
    assert tuple(den2(x).shape) == (2, 1, 2560)
    with pytest.raises(ValueError):
        Denoiser(v, mode="ones")
    with pytest.raises(ValueError):
        Denoiser(v, filter_length=1024, n_overlap=3)


def test_tts_and_synthesizer_denoise_strength(tmp_path):
    from e2e_tts_amd.api import TTS, Synthesizer
    cfg = cfgmod.tiny_config()
    stats = cfgmod.DEFAULT_STATS
    ac = sw.make_acoustic_state(cfg, stats, 4, seed=7, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=8)
    apath, vpath = write_checkpoints(tmp_path, cfg, ac, voc)
    g2p = lambda t: [4 + (ord(c) % 127) for c in t]   # noqa: E731
    tts = TTS(apath, vpath, max_len=60, text_to_sequence=g2p)
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [list(rng.integers(4, 131, n)) for n in (25, 9, 31)]
    plain = tts.inference_ids(seqs, "spk_c", silence_distance=0.01)
    assert tts.engine.denoiser_calibrated is None          # strength 0 never touches the denoiser
    den = tts.inference_ids(seqs, "spk_c", silence_distance=0.01, denoise_strength=0.1)
    assert tts.engine.denoiser_calibrated == (1024, 4, 1024)   # loaded and calibrated at first use
    assert den.dtype == np.int16 and den.shape == plain.shape and (den != plain).any()
    # what it is: set_denoise(0.1) around the same synthesize calls; and the engine's strength is back at 0 afterwards
    np.testing.assert_array_equal(tts.inference_ids(seqs, "spk_c", silence_distance=0.01), plain)
    batches, revert = TTS.pack_sequences(seqs, 60)
    tts.engine.set_denoise(0.1)
    rows, lens = [], []
    for ids, ln in batches:
        pcm, mel_lens, _ = tts.engine.synthesize(ids, ln, np.array([cfgmod.DEFAULT_SPEAKERS["spk_c"]], np.int64))
        rows.extend(list(pcm))
        lens.extend(int(m) for m in mel_lens)
    tts.engine.set_denoise(0.0)
    want = tts._combine_pcm([rows[i] for i in revert.tolist()], [lens[i] for i in revert.tolist()], int(0.01 * 22050))
    np.testing.assert_array_equal(den, want)
    # other weights in the same engine: the next denoised call calibrates again
    from e2e_tts_amd import packer
    bias0 = tts.engine.denoiser_calibrate(None, 88)
    tts.engine.load_weights(packer.pack(tts._dims, ac, sw.make_vocoder_state(cfg, seed=9)))
    assert tts.engine.denoiser_calibrated is None
    tts.inference_ids(seqs[:1], "spk_c", denoise_strength=0.1)
    assert tts.engine.denoiser_calibrated == (1024, 4, 1024)
    tts.engine.denoiser_set_bias(bias0)   # (the engine had a bias all along; what changed is which one)
    with pytest.raises(ValueError):
        tts.inference_ids(seqs, "spk_c", denoise_strength=-1.0)
    # the text path and the service wrapper
    t_plain = tts.inference(["xin chao , viet nam"], "spk_b")
    t_den = tts.inference(["xin chao , viet nam"], "spk_b", denoise_strength=0.2)
    assert t_den.shape == t_plain.shape and (t_den != t_plain).any()
    syn = Synthesizer(apath, vpath, output_dir=str(tmp_path / "out"), max_len=60, text_to_sequence=g2p)
    p0 = syn.synthesis("xin chao , viet nam", save_filepath=str(tmp_path / "out" / "a.wav"), speaker_id="spk_b")
    p1 = syn.synthesis("xin chao , viet nam", save_filepath=str(tmp_path / "out" / "b.wav"), speaker_id="spk_b", denoise_strength=0.2)
    frames = []
    for p in (p0, p1):
        with wave.open(p) as f:
            frames.append(np.frombuffer(f.readframes(f.getnframes()), "<i2"))
    assert frames[0].shape == frames[1].shape and (frames[0] != frames[1]).any()
