"""Per-utterance and per-phoneme controls on the GPU (-m gpu): e2etts_acoustic_ctl / e2etts_synthesize_ctl against the fixtures the
reference produced with tensor controls (tools/make_ctl_goldens.py), directly and through the torch mirror, plus the invariants that
tie the array forms to the scalar entry points bit for bit, and TTS with per-text speakers and controls.

Bars as in test_gpu_parity.py: test_tiny_model_full_trace: durations, mel lengths and bucket indices exact; taps, mel_post and wav
mean-L1 < 1e-5; int16 PCM within 1 LSB on >= 99.9 % of samples; fp32 and bf16x3."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import load_golden, states_for
from e2e_tts_amd import config as cfgmod, synth_weights as sw

pytestmark = pytest.mark.gpu

CTL_CASES = ["tiny_pctl_b3", "tiny_nouv_pctl_b3", "tiny_frame_pctl_b3"]
PRECISIONS = ("fp32", "bf16x3")
WANT = ("dur", "mel_lens", "pitch_idx", "energy_idx", "log_d", "pitch_pred", "energy_pred")
_ENGINES = {}


def engine_for(g, name):
    from e2e_tts_amd.runtime import engine_from_states
    if name not in _ENGINES:
        cfg, ac, voc = states_for(g, name)
        _ENGINES[name] = (cfg, engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, voc, device=0))
    return _ENGINES[name]


def mean_l1(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def engine_controls(g):
    """The controls as the engine takes them: the reference's shapes at the phoneme level; at the frame level the per-phoneme arrays the
    fixture's [B, T] ones were expanded from (the extension rule of include/e2etts.h)."""
    if "p_control_ph" in g:
        p = g["p_control_ph"][..., None] if g["p_control"].ndim == 3 else g["p_control_ph"]
        return g["d_control"], p, g["e_control_ph"]
    return g["d_control"], g["p_control"], g["e_control"]


def full_run(eng, cfg, ids, lens, spk, d, p, e):
    """Every output of one acoustic pass and the vocoder on its resident mel_post: the acoustic outputs, taps, mel, wav, PCM."""
    r = eng.acoustic(ids, lens, spk, d, p, e, want=WANT)
    B, T = r["B"], r["T"]
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    r["mel"], r["mel_post"] = eng.fetch_mel(B, T)
    r["enc_out"] = eng.fetch_tap("enc_out", (B, ids.shape[1], H))
    r["dec_out"] = eng.fetch_tap("dec_out", (B, T, H))
    r["wav"], r["pcm"] = eng.vocoder(None, B, T, wav=True, pcm=True)
    return r


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


@pytest.mark.parametrize("name", CTL_CASES)
def test_fixture_through_acoustic_ctl(name):
    g = load_golden(name)
    cfg, eng = engine_for(g, name)
    spk = np.array([int(g["speaker"])], np.int64)
    d, p, e = engine_controls(g)
    for prec in PRECISIONS:
        eng.set_precision(prec)
        r = full_run(eng, cfg, g["ids"], g["lens"], spk, d, p, e)
        for k in ("dur", "mel_lens", "pitch_idx", "energy_idx"):
            np.testing.assert_array_equal(r[k], g[k], err_msg=f"{k} {prec}")
        for k in ("log_d", "pitch_pred", "energy_pred", "enc_out", "dec_out", "mel", "mel_post", "wav"):
            assert r[k].shape == g[k].shape, k
            assert mean_l1(r[k], g[k]) < 1e-5, (k, prec)
        ref_pcm = (g["wav"] * 32768.0).astype(np.int16)
        assert (np.abs(r["pcm"].astype(np.int32) - ref_pcm.astype(np.int32)) <= 1).mean() >= 0.999, prec
    # the controls decide: the unit controls give other durations
    np.testing.assert_raises(AssertionError, np.testing.assert_array_equal, eng.acoustic(g["ids"], g["lens"], spk)["dur"], g["dur"])


@pytest.mark.parametrize("name", CTL_CASES)
def test_fixture_through_the_torch_mirror(name):
    """UnsupervisedFastSpeech2.inference called with tensors of the shapes the reference got (GPU tensors for d and e, a host tensor for
    p) gives the reference's outputs."""
    import torch
    from e2e_tts_amd.models import UnsupervisedFastSpeech2
    g = load_golden(name)
    cfg, ac, _ = states_for(g, name)
    m = UnsupervisedFastSpeech2(n_symbols=131, n_speakers=4, n_channels=80, config=cfg["models"]["fastspeech2"], stats=cfgmod.DEFAULT_STATS)
    m.load_state_dict(sw.to_torch(ac))
    dev = torch.device("cuda", 0)
    m.eval().to(dev)
    d, p, e = engine_controls(g)
    for prec in PRECISIONS:
        m.engine.set_precision(prec)
        (mel, mel_post, dur), mel_lens = m.inference(speaker=torch.tensor([int(g["speaker"])]), texts=torch.from_numpy(g["ids"]),
                                                     txt_lens=torch.from_numpy(g["lens"]), max_txt_len=g["ids"].shape[1],
                                                     d_control=torch.from_numpy(d).to(dev), p_control=torch.from_numpy(p),
                                                     e_control=torch.from_numpy(e).to(dev))
        np.testing.assert_array_equal(dur.cpu().numpy(), g["dur"])
        np.testing.assert_array_equal(mel_lens.cpu().numpy(), g["mel_lens"])
        assert mean_l1(mel.cpu().numpy(), g["mel"]) < 1e-5, prec
        assert mean_l1(mel_post.cpu().numpy(), g["mel_post"]) < 1e-5, prec


@pytest.mark.parametrize("name", ["tiny_pctl_b3", "tiny_frame_pctl_b3"])
def test_array_forms_equal_the_scalar_forms_bit_for_bit(name):
    """A B * L array uniform per row equals the B form (at the frame level: padded frames included); a B array of one value equals the
    scalar entry point; controls in device memory equal the same values in host memory."""
    import torch
    g = load_golden(name)
    cfg, eng = engine_for(g, name)
    eng.set_precision("fp32")
    ids, lens = g["ids"], g["lens"]
    B, L = ids.shape
    spk = np.array([int(g["speaker"])], np.int64)
    uv = g["p_control"].ndim == 3
    col = lambda v: v[:, None, None] if uv else v[:, None]   # noqa: E731 -- per-utterance pitch control in the reference's shape
    du, pu, eu = np.array([1.2, 0.7, 1.0], np.float32), np.array([0.8, 1.3, 1.1], np.float32), np.array([1.5, 0.6, 0.9], np.float32)
    per_utt = full_run(eng, cfg, ids, lens, spk, du[:, None], col(pu), eu[:, None])
    uniform = full_run(eng, cfg, ids, lens, spk, np.repeat(du[:, None], L, 1), col(pu) * np.ones((1, L) + ((1,) if uv else ()), np.float32),
                       np.repeat(eu[:, None], L, 1))
    assert_same_bits(per_utt, uniform)
    one = np.ones((B, 1), np.float32)
    scalar = full_run(eng, cfg, ids, lens, spk, 1.25, 0.85, 1.15)
    assert_same_bits(full_run(eng, cfg, ids, lens, spk, one * 1.25, col(one[:, 0] * 0.85), one * 1.15), scalar)
    dev = torch.device("cuda", 0)
    d, p, e = engine_controls(g)
    host = full_run(eng, cfg, ids, lens, spk, d, p, e)
    device = full_run(eng, cfg, ids, lens, spk, *(torch.from_numpy(x).to(dev) for x in (d, p, e)))
    assert_same_bits(host, device)


def test_synthesize_ctl_ragged_equals_unragged_on_valid_samples():
    g = load_golden("tiny_pctl_b3")
    cfg, eng = engine_for(g, "tiny_pctl_b3")
    eng.set_precision("fp32")
    spk = np.array([0, 2, 3], np.int64)   # one speaker per row
    d, p, e = engine_controls(g)
    hop = cfg["audio"]["stft"]["hop_length"]
    eng.set_ragged(False)
    a, ml, T = eng.synthesize(g["ids"], g["lens"], spk, d, p, e)
    eng.set_ragged(True)
    b, ml2, T2 = eng.synthesize(g["ids"], g["lens"], spk, d, p, e)
    assert T == T2 and (ml == ml2).all() and (ml < T).any()
    for r, n in enumerate(ml):
        np.testing.assert_array_equal(a[r, :n * hop], b[r, :n * hop])
    # the same PCM as acoustic_ctl + vocoder
    r = eng.acoustic(g["ids"], g["lens"], spk, d, p, e)
    _, pcm = eng.vocoder(None, r["B"], r["T"], wav=False, pcm=True)
    np.testing.assert_array_equal(pcm, a)


def test_rows_with_their_own_controls_equal_each_utterance_alone():
    """A fixed-length batch (uniform-duration weights, equal lengths: no padded rows) whose rows carry different speakers and p / e
    controls gives each row exactly what that utterance gives alone at B = 1 with its scalars."""
    from e2e_tts_amd.runtime import engine_from_states
    cfg = cfgmod.tiny_config()
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=1234, mode="fixed")
    voc = sw.make_vocoder_state(cfg, seed=4321)
    eng = engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, voc, device=0)
    rng = np.random.Generator(np.random.PCG64(5))
    B, L = 3, 16
    ids = rng.integers(4, 131, size=(B, L)).astype(np.int64)
    lens = np.full((B,), L, np.int64)
    spk = np.array([1, 3, 0], np.int64)
    pc, ec = np.array([0.7, 1.0, 1.4], np.float32), np.array([1.3, 0.6, 1.0], np.float32)
    batch = full_run(eng, cfg, ids, lens, spk, 1.0, pc[:, None, None], ec[:, None])
    pcm_b, ml_b, _ = eng.synthesize(ids, lens, spk, 1.0, pc[:, None, None], ec[:, None])
    assert len(set(batch["mel_lens"].tolist())) == 1
    for b in range(B):
        one = full_run(eng, cfg, ids[b:b + 1], lens[b:b + 1], spk[b:b + 1], 1.0, float(pc[b]), float(ec[b]))
        for k in ("dur", "mel_lens", "pitch_idx", "energy_idx", "pitch_pred", "energy_pred", "mel", "mel_post", "dec_out", "wav", "pcm"):
            np.testing.assert_array_equal(batch[k][b], one[k][0], err_msg=f"{k} row {b}")
        np.testing.assert_array_equal(pcm_b[b], one["pcm"][0])
    assert len({batch["pitch_idx"][b].tobytes() for b in range(B)}) == B   # the rows' controls did differ


def test_wrong_count_is_einval_and_the_engine_stays_usable():
    g = load_golden("tiny_pctl_b3")
    cfg, eng = engine_for(g, "tiny_pctl_b3")
    eng.set_precision("fp32")
    spk = np.array([int(g["speaker"])], np.int64)
    d, p, e = engine_controls(g)
    ref = eng.acoustic(g["ids"], g["lens"], spk, d, p, e, want=WANT)
    B, L = g["ids"].shape
    ids, lens = np.ascontiguousarray(g["ids"]), np.ascontiguousarray(g["lens"])
    vals = np.ones(B * L + 1, np.float32)
    T = C.c_int(0)
    pcm = np.empty(1, np.int16)
    for n in (0, 2, B + 1, B * L - 1, B * L + 1, -1):
        rc = eng.lib.e2etts_acoustic_ctl(eng._h, ids.ctypes.data, lens.ctypes.data, B, L, spk.ctypes.data, 1, None, 0,
                                         vals.ctypes.data, n, None, 0, None, None, C.byref(T), None, None, None, None, None)
        assert rc == -1, n
        assert b"p_control" in eng.lib.e2etts_last_error(eng._h)
        rc = eng.lib.e2etts_synthesize_ctl(eng._h, ids.ctypes.data, lens.ctypes.data, B, L, spk.ctypes.data, 1, vals.ctypes.data, n,
                                           None, 0, None, 0, pcm.ctypes.data, pcm.size, None, C.byref(T))
        assert rc == -1, n
        r = eng.acoustic(g["ids"], g["lens"], spk, d, p, e, want=WANT)
        for k in WANT + ("T",):
            np.testing.assert_array_equal(r[k], ref[k], err_msg=k)


def test_repeated_calls_allocate_nothing():
    g = load_golden("tiny_frame_pctl_b3")
    cfg, eng = engine_for(g, "tiny_frame_pctl_b3")
    spk = np.array([int(g["speaker"])], np.int64)
    d, p, e = engine_controls(g)
    B = g["ids"].shape[0]

    def calls():
        eng.acoustic(g["ids"], g["lens"], spk, d, p, e, want=WANT)
        eng.synthesize(g["ids"], g["lens"], spk, d[:, :1], p[:, :1], e[:, :1])
        eng.synthesize(g["ids"], g["lens"], np.arange(B, dtype=np.int64), np.float32(1.1) * np.ones(1, np.float32), 0.9, e)
    calls()
    before = eng.device_bytes()
    for _ in range(3):
        calls()
    assert eng.device_bytes() == before


def write_checkpoints(tmp_path, cfg, ac, voc):
    import torch
    import yaml
    d = tmp_path / "exps" / "acoustic"
    v = tmp_path / "exps" / "vocoder"
    d.mkdir(parents=True)
    v.mkdir(parents=True)
    torch.save({"state_dict": sw.to_torch(ac), "optimizer": {}}, d / "statedict.pt")
    torch.save({"state_dict": sw.to_torch(voc)}, v / "statedict.pt")
    yaml.safe_dump(dict(cfg), open(d / "config.yaml", "w"))
    json.dump(cfgmod.DEFAULT_SPEAKERS, open(d / "speakers.json", "w"))
    json.dump(cfgmod.DEFAULT_STATS, open(d / "stats.json", "w"))
    return str(d / "statedict.pt"), str(v / "statedict.pt")


def test_tts_per_text_speakers_and_controls(tmp_path):
    from e2e_tts_amd.api import TTS
    cfg = cfgmod.tiny_config()
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=7, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=8)
    apath, vpath = write_checkpoints(tmp_path, cfg, ac, voc)
    tts = TTS(apath, vpath, max_len=40, text_to_sequence=lambda t: [4 + (ord(c) % 127) for c in t])
    # every piece a distinct length, so that the length sort -- and with it every batch -- is the same for any order of the texts
    texts = ["xin chao viet", " , ".join(["mot hai ba bon nam sau", "bay tam chin muoi mot", "hai ba bon nam sau bay tam"]),
             "tieng noi tong hop", "am"]
    spk = ["spk_b", "spk_d", "hn_minhphuong", "spk_c"]
    d, p, e = [1.2, 0.8, 1.0, 1.5], [0.9, 1.3, 0.6, 1.0], [1.1, 0.7, 1.4, 1.0]
    pieces, owners = tts.arrange_text_owners(texts, tts.max_len)
    assert len(pieces) > len(texts) and len({len(x) for x in pieces}) == len(pieces)
    silence = 0.01
    gap = int(silence * tts.sample_rate)

    captured = []
    orig = tts._combine_pcm

    def capture(pcms, lengths, distance):
        captured.append([np.asarray(x[:int(n) * tts.hop_length]) for x, n in zip(pcms, lengths)])
        return orig(pcms, lengths, distance)
    tts._combine_pcm = capture
    out = tts.inference(texts, spk, p, e, d, silence_distance=silence)
    perm = [2, 0, 3, 1]
    out_p = tts.inference([texts[i] for i in perm], [spk[i] for i in perm], [p[i] for i in perm], [e[i] for i in perm],
                          [d[i] for i in perm], silence_distance=silence)
    assert out.size == out_p.size and not np.array_equal(out, out_p)
    per_text = lambda segs, own: [np.concatenate([s for s, o in zip(segs, own) if o == i]) for i in range(len(texts))]   # noqa: E731
    _, owners_p = tts.arrange_text_owners([texts[i] for i in perm], tts.max_len)
    a, b = per_text(captured[0], owners), per_text(captured[1], owners_p)
    for j, i in enumerate(perm):
        np.testing.assert_array_equal(b[j], a[i])
    assert sum(x.size for x in captured[0]) + gap * len(pieces) == out.size
    # all-equal lists are the scalar call, bit for bit; the per-text settings did matter
    same = tts.inference(texts, ["spk_b"] * 4, [1.1] * 4, [0.9] * 4, [1.2] * 4, silence_distance=silence)
    scal = tts.inference(texts, "spk_b", 1.1, 0.9, 1.2, silence_distance=silence)
    np.testing.assert_array_equal(same, scal)
    assert not np.array_equal(a[0], per_text(captured[2], owners)[0])
