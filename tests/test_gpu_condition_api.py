"""Recording conditioning through the public interfaces: condition= of UnsupervisedFastSpeech2.align_audio / forward_audio (alone and behind
wav_rate=) and condition.normalize_signal, against the plain-integer definition (tests/condition_ref.py).  Everything is compared bit for
bit: the conditioned PCM is exact, and the mel library is handed the same int16 samples either way."""
import numpy as np
import pytest

from conftest import load_golden
import condition_ref as cr
import mel_ref as mr
from aligner_cases import fixture_state
from e2e_tts_amd import condition as cd, config as cfgmod, resample as rs, synth_weights as sw

pytestmark = pytest.mark.gpu

LOUD = -23.0
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
        stft = models.TorchSTFT(int(g["n_fft"]), int(g["hop"]), int(g["win_length"]), int(g["n_mel"]), int(g["sr"]), float(g["fmin"]), float(g["fmax"]),
                                device="cuda:0", mel_basis=g["mel_basis"])
        pcm, nv = g["pcm"], np.asarray(g["n_valid"], np.int64)
        # studio recordings: 180 ms of room tone in front, 130 ms behind
        rate = int(g["sr"])
        rng = np.random.Generator(np.random.PCG64(5))
        lead, tail = cr.pos(180, rate), cr.pos(130, rate)
        rows = [np.concatenate([rng.integers(-30, 31, lead), pcm[b, :nv[b]], rng.integers(-30, 31, tail)]).astype(np.int16) for b in range(len(nv))]
        _M.update(g=g, m=m, stft=stft, rows=rows, rate=rate)
    return _M


def conditioned(rows, rate, trim, loud):
    """The ref-conditioned batch: ([B, width] int16, n_out)"""
    out = [cr.normalize(r, rate, trim, loud) for r in rows]
    return cr.batch([o["pcm"] for o in out])


def same(a, b):
    return all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))


def test_condition_none_is_todays_path():
    M = model()
    g, m, stft = M["g"], M["m"], M["stft"]
    x, lens = cr.batch(M["rows"])
    args = (g["speakers"], g["ids"], g["txt_lens"], x, lens)
    assert same(m.align_audio(*args, stft=stft, return_energy=True), m.align_audio(*args, stft=stft, return_energy=True, condition=None))
    audio = mr.fixture_audio(g)                                                                      # float32, as before
    args = (g["speakers"], g["ids"], g["txt_lens"], audio, g["n_valid"])
    assert same(m.align_audio(*args, stft=stft), m.align_audio(*args, stft=stft, condition=None))
    with pytest.raises(ValueError, match="int16"):
        m.align_audio(*args, stft=stft, condition=dict(trim="reference"))                            # float32 without resampling
    with pytest.raises(ValueError, match="unknown keys"):
        m.align_audio(g["speakers"], g["ids"], g["txt_lens"], x, lens, stft=stft, condition=dict(trimm="reference"))


@pytest.mark.parametrize("trim,loud", [("reference", LOUD), ("both", None)])
def test_align_audio_conditions_on_the_device(trim, loud):
    import torch
    M = model()
    g, m, stft, rate = M["g"], M["m"], M["stft"], M["rate"]
    x, lens = cr.batch(M["rows"])
    want, n_out = conditioned(M["rows"], rate, trim, loud)
    assert (n_out < lens).all()                                                                      # the lead (and with "both" the tail) is gone
    # the chain's hand-over: the mel of the conditioner's resident rows equals the mel of the ref-conditioned array passed in directly
    c = cd.Conditioner(rate)
    r = c.normalize(x, lens, trim=trim, loudness_dBFS=loud, want=("pcm",))
    assert np.array_equal(r["n_out"], n_out) and np.array_equal(r["pcm"], want)
    a = stft.frontend.forward(c.resident()[0], r["n_out"], want=("mel", "energy"))
    mel_a, en_a, ml_a = a["mel"].copy(), a["energy"].copy(), a["mel_lens"].copy()
    b = stft.frontend.forward(want, n_out, want=("mel", "energy"))
    assert np.array_equal(ml_a, b["mel_lens"]) and np.array_equal(ml_a, n_out // int(g["hop"]))
    assert np.array_equal(mel_a, b["mel"]) and np.array_equal(en_a, b["energy"])
    c.close()
    # align_audio: conditioned on the device == the ref-conditioned array handed over
    spk, ids, tl = g["speakers"], g["ids"], g["txt_lens"]
    cond = dict(trim=trim, loudness_dBFS=loud)
    direct = m.align_audio(spk, ids, tl, want, n_out, stft=stft, return_energy=True)
    for src in (x, torch.from_numpy(x).cuda()):
        got = m.align_audio(spk, ids, tl, src, lens, stft=stft, return_energy=True, condition=cond)
        assert same(got, direct)
    assert np.array_equal(direct[2].sum(1).cpu().numpy(), (n_out // int(g["hop"])).astype(np.float32))   # mel_lens follow from n_out
    # stereo: both channels the same recording: the downmix gives the recording back
    st = np.stack([x, x], 2)
    assert np.array_equal(np.stack([cr.downmix(s) for s in st]), x)
    assert same(m.align_audio(spk, ids, tl, st, lens, stft=stft, return_energy=True, condition=dict(cond, channels=2)), direct)
    if trim == "reference":
        fa = m.forward_audio(spk, ids, tl, x, lens, condition=cond)
        fd = m.forward_audio(spk, ids, tl, want, n_out)
        assert same(fa[0][:2], fd[0][:2]) and np.array_equal(fa[0][7].cpu().numpy(), fd[0][7].cpu().numpy())


def test_wav_rate_chain():
    """44.1 kHz recordings: resampled on the device, its int16 output conditioned where it lies == the same steps made one by one."""
    M = model()
    g, m, stft, rate = M["g"], M["m"], M["stft"], M["rate"]
    up_taps = rs.design(rate, 2 * rate)[0]
    import resample_ref as rr
    up_rows = [np.clip(np.round(rr.resample_f64(r.astype(np.float32) / 32768, up_taps, 2, 1) * 32768), -32768, 32767).astype(np.int16) for r in M["rows"]]
    up, up_lens = cr.batch(up_rows)
    down = rs.Resampler(2 * rate, rate)
    d = down.forward(up, n_valid=up_lens, want=("pcm",))
    rows = [d["pcm"][b, :int(d["n_out"][b])] for b in range(len(up_rows))]                              # the resampler's int16 output
    down.close()
    want, n_out = conditioned(rows, rate, "reference", LOUD)
    assert (n_out < d["n_out"]).all()
    spk, ids, tl = g["speakers"], g["ids"], g["txt_lens"]
    direct = m.align_audio(spk, ids, tl, want, n_out, stft=stft, return_energy=True)
    cond = dict(trim="reference", loudness_dBFS=LOUD)
    assert same(m.align_audio(spk, ids, tl, up, up_lens, stft=stft, return_energy=True, wav_rate=2 * rate, condition=cond), direct)
    upf = up.astype(np.float32) / np.float32(32768.0)                                                  # float32 is taken behind the resampler
    assert same(m.align_audio(spk, ids, tl, upf, up_lens, stft=stft, return_energy=True, wav_rate=2 * rate, condition=cond), direct)


def test_normalize_signal():
    M = model()
    rate, row = M["rate"], M["rows"][0]
    e = cr.normalize(row, rate, "reference", LOUD)
    out, r2 = cd.normalize_signal(row, rate, silence_threshold=-35, loudness_dBFS=LOUD)                 # any truthy threshold means -50
    assert r2 == rate and out.dtype == np.int16 and np.array_equal(out, e["pcm"])
    out, _ = cd.normalize_signal(row, rate)                                                            # nothing asked for
    assert np.array_equal(out, row)
    out, _ = cd.normalize_signal(row, rate, loudness_dBFS=LOUD)                                        # loudness alone: unsliced
    assert np.array_equal(out, cr.normalize(row, rate, None, LOUD)["pcm"])
    st = np.stack([row.astype(np.int32) + 3, row.astype(np.int32) - 4], 1).astype(np.int16)            # odd sums: the floor of the downmix
    mono = cr.downmix(st)
    out, _ = cd.normalize_signal(st, rate, channels=1, silence_threshold=True, loudness_dBFS=LOUD)
    assert np.array_equal(out, cr.normalize(mono, rate, "reference", LOUD)["pcm"])
    # the reference's order: channels, rate, silence, loudness
    down = rs.Resampler(rate, 16000)
    d = down.forward(mono[None], want=("pcm",))
    mid = d["pcm"][0, :int(d["n_out"][0])]
    down.close()
    out, r2 = cd.normalize_signal(st, rate, channels=1, sr=16000, silence_threshold=True, loudness_dBFS=LOUD)
    assert r2 == 16000 and np.array_equal(out, cr.normalize(mid, 16000, "reference", LOUD)["pcm"])
