"""The pitch tracker through the public interfaces: UnsupervisedFastSpeech2.forward_audio(p_targets="extract") against the same targets
made step by step on the host (PitchTracker + models.f0_targets) and handed in, bit for bit -- plain, behind wav_rate= and behind
condition= --, models.extract_f0, and the refusals that come before any launch."""
import numpy as np
import pytest

from conftest import load_golden
import mel_ref as mr
from aligner_cases import fixture_state
from e2e_tts_amd import condition as cd, config as cfgmod, f0 as f0lib, resample as rs, synth_weights as sw
from e2e_tts_amd.models import f0_targets

pytestmark = pytest.mark.gpu

_M = {}


def model():
    if not _M:
        from e2e_tts_amd import models
        g = load_golden(mr.ALIGN_FIXTURE)
        cfg = cfgmod.tiny_config()
        fs = cfg["models"]["fastspeech2"]
        state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=3, mode="varied")
        state.update(fixture_state(g))
        m = models.UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0)
        m.load_state_dict(sw.to_torch(state))
        m.engine.set_precision("fp32", "fp32")
        rate, hop = int(g["sr"]), int(g["hop"])
        assert (rate, hop) == (22050, 256)
        # voiced recordings of the fixture's lengths: the fixture's noise plus a tone with pauses, so that the targets hold both kinds of frame
        pcm, nv = g["pcm"].astype(np.int64), np.asarray(g["n_valid"], np.int64)
        t = np.arange(pcm.shape[1]) / rate
        for b in range(pcm.shape[0]):
            tone = 6000.0 * np.sin(2 * np.pi * (140.0 + 60.0 * b) * t) * (np.sin(2 * np.pi * 1.7 * t + b) > -0.4)
            pcm[b] = pcm[b] // 8 + np.rint(tone).astype(np.int64)
            pcm[b, nv[b]:] = 0
        _M.update(g=g, m=m, pcm=np.clip(pcm, -32768, 32767).astype(np.int16), nv=nv, rate=rate, hop=hop, trk=f0lib.PitchTracker(rate, hop))
    return _M


def host_targets(trk, x, lens, T):
    """PitchTracker + f0_targets on the host -> {"f0", "uv"} [B, T] float32, zeros past a row's frames"""
    r = trk.forward(x, lens)
    assert r["T"] == T
    f0, uv = np.zeros((len(lens), T), np.float32), np.zeros((len(lens), T), np.float32)
    for b, n in enumerate(r["lens"]):
        a, u = f0_targets(r["f0"][b, :n].astype(np.float64), cfgmod.DEFAULT_STATS)
        f0[b, :n], uv[b, :n] = a.astype(np.float32), u
    return {"f0": f0, "uv": uv}, r["f0"]


def same(a, b):
    (ma, pa, *_), (pra, _) = a
    (mb, pb, *_), (prb, _) = b
    return all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in ((ma, mb), (pa, pb), (pra["f0"], prb["f0"]), (pra["uv"], prb["uv"])))


def test_extract_equals_the_targets_made_on_the_host():
    M = model()
    g, m, pcm, nv, trk = M["g"], M["m"], M["pcm"], M["nv"], M["trk"]
    args = (g["speakers"], g["ids"], g["txt_lens"])
    T = int(nv.max()) // M["hop"]
    tg, track = host_targets(trk, pcm, nv, T)
    assert (track != 0).any() and (track == 0).any()                                  # voiced and unvoiced frames
    for step in (0, 10 ** 9):
        assert same(m.forward_audio(*args, pcm, nv, p_targets="extract", step=step), m.forward_audio(*args, pcm, nv, p_targets=tg, step=step))
    import torch
    assert same(m.forward_audio(*args, torch.from_numpy(pcm).cuda(), nv, p_targets="extract"), m.forward_audio(*args, pcm, nv, p_targets=tg))
    # p_targets=None is what it was: the prediction is embedded, no target comes back
    a, b = m.forward_audio(*args, pcm, nv), m.forward_audio(*args, pcm, nv, p_targets=None)
    assert a[1][0] is None and b[1][0] is None and np.array_equal(a[0][1].cpu().numpy(), b[0][1].cpu().numpy())
    assert not np.array_equal(a[0][1].cpu().numpy(), m.forward_audio(*args, pcm, nv, p_targets="extract")[0][1].cpu().numpy())


def test_extract_behind_wav_rate():
    M = model()
    g, m, pcm, nv, rate, trk = M["g"], M["m"], M["pcm"], M["nv"], M["rate"], M["trk"]
    args = (g["speakers"], g["ids"], g["txt_lens"])
    up = rs.Resampler(rate, 44100)
    u = up.forward(pcm, n_valid=nv, want=("pcm",))
    up.close()
    x44, n44 = u["pcm"], u["n_out"]
    down = rs.Resampler(44100, rate)
    d = down.forward(x44, n_valid=n44, want=("wav",))                                  # what forward_audio's resampler hands the mel library
    down.close()
    T = int(d["n_out"].max()) // M["hop"]
    tg, _ = host_targets(trk, d["wav"], d["n_out"], T)
    assert same(m.forward_audio(*args, x44, n44, p_targets="extract", wav_rate=44100), m.forward_audio(*args, x44, n44, p_targets=tg, wav_rate=44100))


def test_extract_behind_condition():
    M = model()
    g, m, pcm, nv, rate, trk = M["g"], M["m"], M["pcm"], M["nv"], M["rate"], M["trk"]
    args = (g["speakers"], g["ids"], g["txt_lens"])
    cond = dict(trim="reference", loudness_dBFS=-23.0)
    c = cd.Conditioner(rate)
    r = c.normalize(pcm, nv, trim="reference", loudness_dBFS=-23.0, want=("pcm",))
    c.close()
    T = int(r["n_out"].max()) // M["hop"]
    tg, _ = host_targets(trk, r["pcm"], r["n_out"], T)
    assert same(m.forward_audio(*args, pcm, nv, p_targets="extract", condition=cond), m.forward_audio(*args, pcm, nv, p_targets=tg, condition=cond))


def test_extract_f0_lies_on_the_mel_grid():
    from e2e_tts_amd import models
    M = model()
    pcm, nv, rate, hop, trk = M["pcm"], M["nv"], M["rate"], M["hop"], M["trk"]
    n = int(nv[1])
    mel_len = n // hop
    f0, coarse = models.extract_f0(pcm[1, :n], mel_len, rate, hop, with_pitch=True)
    assert f0.shape == (mel_len,) and f0.dtype == np.float64 and coarse.shape == (mel_len,)
    assert np.array_equal(f0.astype(np.float32), trk.forward(pcm[1:2, :n])["f0"][0])
    assert coarse.min() >= 1 and coarse.max() <= 255 and (coarse[f0 == 0] == 1).all()
    assert np.array_equal(models.extract_f0(pcm[1, :n].astype(np.float32) / np.float32(32768.0), mel_len, rate, hop), f0)   # int16 is the same signal / 32768


def test_bad_arguments_raise_before_any_launch():
    from e2e_tts_amd import models
    M = model()
    g, m, pcm, nv, trk = M["g"], M["m"], M["pcm"], M["nv"], M["trk"]
    args = (g["speakers"], g["ids"], g["txt_lens"])
    with pytest.raises(ValueError, match="'extract'"):
        m.forward_audio(*args, pcm, nv, p_targets="praat")
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    fs["variance"]["variance_embedding"]["use_uv"] = False
    nouv = models.UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0)
    with pytest.raises(ValueError, match="use_uv"):                                    # before the aligner, the mel or the tracker is touched:
        nouv.forward_audio(*args, pcm, nv, p_targets="extract")                        # this model has no state loaded at all
    before = trk.device_bytes()
    bad = nv.copy()
    bad[0] = pcm.shape[1] + 1
    with pytest.raises(ValueError, match="n_valid"):
        trk.forward(pcm, bad)
    with pytest.raises(ValueError, match="frame"):
        trk.forward(pcm[:, :100])                                                      # shorter than one hop
    with pytest.raises(TypeError):
        trk.forward(pcm.astype(np.float64))
    with pytest.raises(ValueError, match="pitch_quantization"):
        trk.targets(cfgmod.DEFAULT_STATS, "mel")
    trk.forward(pcm, nv)
    with pytest.raises(ValueError, match="std"):
        trk.targets({"f0": {"mean": 0.0, "std": 0.0}})
    assert trk.device_bytes() >= before
    f0 = trk.forward(pcm, nv)["f0"]                                                    # the handle stays usable
    assert np.isfinite(f0).all()
    with pytest.raises(ValueError, match="tau_min"):
        f0lib.PitchTracker(22050, 256, ceiling=30000.0)
    with pytest.raises(ValueError, match="LDS"):
        f0lib.PitchTracker(48000, 512, floor=40.0)                                     # W = 3601: refused, the limit is stated
    with pytest.raises(ValueError, match="max_candidates"):
        f0lib.PitchTracker(22050, 256, max_candidates=17)
