"""GPU tests (-m gpu) of ``attn_prior="device"`` on the model level (models.UnsupervisedFastSpeech2.align / align_audio): the prior is
generated inside the aligner's attention pass, and the result is the one of the same call handed ``Aligner.prior``'s tensor explicitly,
bit for bit; on the reference's fixture the durations and the hard map are the goldens."""
import numpy as np
import pytest

from conftest import load_golden
from aligner_cases import fixture_state
from e2e_tts_amd import config as cfgmod, synth_weights as sw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_and_fixture():
    import torch  # noqa: F401
    from e2e_tts_amd.models import UnsupervisedFastSpeech2
    g = load_golden("aligner_tiny_b3")
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    fs["encoder_hidden"] = fs["decoder_hidden"] = int(g["hidden"])
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=3, mode="varied")
    state.update(fixture_state(g))
    m = UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0)
    m.load_state_dict(sw.to_torch(state))
    return m, g


def same_bits(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32)) for x, y in zip(a, b))


def test_model_align_with_the_device_prior(model_and_fixture):
    import torch
    m, g = model_and_fixture
    args = [torch.from_numpy(g[k]) for k in ("speakers", "ids", "txt_lens", "mel", "mel_lens")]
    soft, hard, dur, logprob = out = m.align(*args, attn_prior="device")
    B, T, L = g["attn"].shape
    assert soft.shape == hard.shape == logprob.shape == (B, 1, T, L) and dur.shape == (B, L) and soft.is_cuda
    assert np.array_equal(dur.cpu().numpy(), g["dur"])
    assert np.array_equal(hard[:, 0].cpu().numpy(), g["attn_hard"].astype(np.float32))
    prior = torch.empty((B, T, L), dtype=torch.float32, device="cuda")
    m._ensure_aligner()[0].encoder.prior(g["txt_lens"], g["mel_lens"], T, L, out=prior)
    assert same_bits(out, m.align(*args, attn_prior=prior))
    with pytest.raises(ValueError, match="device"):
        m.align(*args, attn_prior="host")


def test_align_audio_with_the_device_prior(model_and_fixture):
    import torch
    m, g = model_and_fixture
    rng = np.random.Generator(np.random.PCG64(41))
    wav_lens = np.array([4000, 2700], np.int64)
    wavs = (rng.standard_normal((2, 4000)) * 0.1).astype(np.float32)
    wavs[1, 2700:] = 0
    ids, tl, spk = torch.from_numpy(g["ids"][:2, :9].copy()), torch.tensor([9, 5]), torch.from_numpy(g["speakers"][:2])
    ids[1, 5:] = 0
    out = m.align_audio(spk, ids, tl, wavs, wav_lens, attn_prior="device")
    B, _, T, L = out[0].shape
    hop = m._default_stft().frontend.hop
    ml = wav_lens // hop
    assert (B, T, L) == (2, int(ml.max()), 9) and ml[1] < T
    prior = m._ensure_aligner()[0].encoder.prior(tl.numpy(), ml, T, L)
    assert prior[1, :ml[1], :5].all() and not prior[1, ml[1]:].any() and not prior[1, :, 5:].any()
    assert same_bits(out, m.align_audio(spk, ids, tl, wavs, wav_lens, attn_prior=prior))
    assert float(out[2].sum()) == float(ml.sum())          # every frame belongs to a phoneme
