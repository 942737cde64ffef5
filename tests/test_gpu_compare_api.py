"""The comparison library through the public interfaces: compare.compare_audio on constructed signals, compare.Comparator fed from what
lies resident in a MelFrontend / PitchTracker against the same call fed host arrays, TTS.evaluate_ids against the chain made by hand,
inference_ids against its batches assembled by hand (the factored batch loop returns the same bytes), and the frame-synchronous
comparison of forward_audio's teacher-forced mel_post with the recording's own mel."""
import numpy as np
import pytest

import compare_cases as cc
from e2e_tts_amd import compare as cmplib, config as cfgmod, f0 as f0lib, mel as mellib, synth_weights as sw

pytestmark = pytest.mark.gpu

SR, HOP, N_FFT, N_MEL = 22050, 256, 1024, 80


def bitwise(a, b):
    """Two lists of result dicts, equal bit for bit (NaN equal to NaN)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k
    return True


def test_a_signal_against_itself():
    lens = np.array([HOP * 70 + 13, HOP * 41])
    x = np.stack([cc.harmonic(int(lens[0]), SR, 150.0, 1), cc.harmonic(int(lens[0]), SR, 220.0, 2)])
    for mode in ("dtw", "sync"):
        res = cmplib.compare_audio(x, lens, x.copy(), lens, SR, HOP, mode=mode, return_path=True)
        for r, n in zip(res, lens // HOP):
            assert r["status"] == 0 and r["n_path"] == n and r["mcd_db"] == 0.0 and r["dist_total"] == 0.0 and r["mel_l1"] == 0.0
            assert np.array_equal(r["path"], np.stack([np.arange(n), np.arange(n)], 1))
            assert r["n_voiced_both"] > n // 2 and r["n_vuv_mismatch"] == 0 and r["f0_rmse_hz"] == 0.0 and r["f0_rmse_cents"] == 0.0
    pcm = np.rint(x * 20000).astype(np.int16)
    assert cmplib.compare_audio(pcm, lens, pcm, lens, SR, HOP, with_f0=False)[0]["mcd_db"] == 0.0


def test_a_repeated_segment_is_walked_horizontally():
    """A: a rising chirp, a steady harmonic tone, a falling chirp.  B: the same with the steady tone 20 frames longer.  The tone's period
    divides the hop, so every frame whose window lies inside it is the same frame bit for bit, and the insert changes no window that
    reaches a chirp: the path is the diagonal with one horizontal run of Tb - Ta cells inside the tone, at distance 0:
    n_path = Ta + (Tb - Ta), no vertical step."""
    f0 = 2 * SR / HOP                                   # 172.27 Hz: two periods a hop

    def tone(n):
        t = np.arange(n)
        return 0.3 * sum(a * np.sin(2 * np.pi * (k + 1) * f0 * t / SR) for k, a in enumerate([1.0, 0.5, 0.3])) / 1.8

    def chirp(n, fa, fb, seed):
        f = np.linspace(fa, fb, n)
        ph = 2 * np.pi * np.cumsum(f) / SR
        return 0.3 * (np.sin(ph) + 0.4 * np.sin(2 * ph)) / 1.4 + 0.01 * np.random.default_rng(seed).standard_normal(n)

    n1, ns, n2, extra = 30 * HOP, 40 * HOP, 25 * HOP, 20 * HOP
    c1, c2 = chirp(n1, 120.0, 260.0, 1), chirp(n2, 300.0, 140.0, 2)
    a = np.concatenate([c1, tone(ns), c2]).astype(np.float32)
    b = np.concatenate([c1, tone(ns + extra), c2]).astype(np.float32)
    Ta, Tb = a.size // HOP, b.size // HOP
    wa = np.zeros((1, b.size), np.float32)
    wa[0, :a.size] = a
    r = cmplib.compare_audio(wa, [a.size], b[None], [b.size], SR, HOP, return_path=True)[0]
    steps = np.diff(r["path"], axis=0)
    horizontal = np.flatnonzero((steps[:, 0] == 0) & (steps[:, 1] == 1))
    print(f"Ta {Ta} Tb {Tb} n_path {r['n_path']} dist_total {r['dist_total']:.3e} horizontal run at i = {r['path'][horizontal[0], 0] if horizontal.size else None}")
    assert r["n_path"] == Ta + (Tb - Ta) and not ((steps[:, 0] == 1) & (steps[:, 1] == 0)).any()
    assert horizontal.size == Tb - Ta and (np.diff(horizontal) == 1).all()          # one run
    reach = N_FFT // HOP                                                             # frames an analysis window spans
    i_run = r["path"][horizontal[0], 0]
    assert 30 - reach <= i_run <= 30 + 40 + reach                                    # inside the tone, within the window's reach
    assert r["dist_total"] == 0.0 and r["mcd_db"] == 0.0 and r["f0_rmse_hz"] < 1.0


def test_resident_inputs_equal_host_arrays():
    """The comparator reading the mel front-end's and the pitch tracker's HBM equals the same call fed their outputs as host arrays
    and as torch tensors on the GPU, bit for bit."""
    import torch
    lens_a, lens_b = np.array([HOP * 50, HOP * 33 + 100]), np.array([HOP * 44 + 7, HOP * 52])
    xa = np.stack([cc.harmonic(HOP * 52, SR, 140.0, 3), cc.harmonic(HOP * 52, SR, 200.0, 4)])
    xb = np.stack([cc.harmonic(HOP * 52, SR, 150.0, 5), cc.harmonic(HOP * 52, SR, 190.0, 6)])
    fe = mellib.MelFrontend(N_FFT, HOP, N_MEL)
    fe.load(mellib.dft_basis(N_FFT), mellib.mel_filterbank(SR, N_FFT, N_MEL, 0.0, 8000.0))
    trk = f0lib.PitchTracker(SR, HOP)
    c_res, c_host, c_dev = cmplib.Comparator(N_MEL), cmplib.Comparator(N_MEL), cmplib.Comparator(N_MEL)
    for side, x, ln in (("a", xa, lens_a), ("b", xb, lens_b)):
        r = fe.forward(x, ln)
        t = trk.forward(x, ln)
        c_res.set_mels(side, fe, r["mel_lens"], trk)
        c_host.set_mels(side, r["mel"], r["mel_lens"], t["f0"])
        c_dev.set_mels(side, torch.from_numpy(r["mel"]).cuda(), torch.from_numpy(r["mel_lens"]), torch.from_numpy(t["f0"]).cuda())
    assert np.array_equal(c_res.features("a"), c_host.features("a")) and np.array_equal(c_res.features("b"), c_dev.features("b"))
    for mode, band in (("dtw", None), ("dtw", 4), ("sync", None)):
        want = c_host.run(mode, band, return_path=True)
        assert bitwise(c_res.run(mode, band, return_path=True), want) and bitwise(c_dev.run(mode, band, return_path=True), want)
        assert all(r["status"] == 0 and r["mcd_db"] > 0 and r["n_voiced_both"] > 0 for r in want)
    # and compare_audio is that chain
    assert bitwise(cmplib.compare_audio(xa, lens_a, xb, lens_b, SR, HOP, return_path=True), c_host.run(return_path=True))
    for c in (c_res, c_host, c_dev, fe, trk):
        c.close()


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    from test_gpu_denoiser_api import write_checkpoints
    from e2e_tts_amd.api import TTS
    cfg = cfgmod.tiny_config()
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=7, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=8)
    apath, vpath = write_checkpoints(tmp_path_factory.mktemp("ckpt"), cfg, ac, voc)
    return TTS(apath, vpath, max_len=60, text_to_sequence=lambda t: [4 + (ord(c) % 127) for c in t])


def by_hand(tts, seqs, speaker):
    """inference_ids' utterances from the engine, batch by batch: (pcm rows, mel lengths) in request order."""
    from e2e_tts_amd.api import TTS
    batches, revert = TTS.pack_sequences(seqs, tts.max_len)
    pcms, lens = [], []
    for ids, ln in batches:
        pcm, mel_lens, _ = tts.engine.synthesize(ids, ln, np.array([cfgmod.DEFAULT_SPEAKERS[speaker]], np.int64))
        pcms.extend(np.array(p) for p in pcm)
        lens.extend(int(m) for m in mel_lens)
    return [pcms[i] for i in revert.tolist()], [lens[i] for i in revert.tolist()]


def test_inference_ids_is_unchanged(tts):
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [list(rng.integers(4, 131, n)) for n in (25, 9, 31, 40, 12)]
    pcms, lens = by_hand(tts, seqs, "spk_c")
    gap = int(0.5 * tts.sample_rate)
    want = np.concatenate([np.concatenate([p[:n * tts.hop_length], np.zeros(gap, np.int16)]) for p, n in zip(pcms, lens)])
    got = tts.inference_ids(seqs, "spk_c")
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(tts.inference_ids(seqs, ["spk_c"] * 5, pitch_control=[1.0] * 5), want)
    assert np.array_equal(tts.inference_ids(seqs, "spk_c", output_rate=tts.sample_rate, denoise_strength=0.0), want)


def test_evaluate_ids_equals_the_chain_made_by_hand(tts):
    rng = np.random.Generator(np.random.PCG64(12))
    seqs = [list(rng.integers(4, 131, n)) for n in (25, 9, 31)]
    rec_lens = np.array([HOP * 60 + 5, HOP * 35, HOP * 48])
    rec = np.stack([np.rint(12000 * cc.harmonic(HOP * 61, SR, f, k)).astype(np.int16) for k, f in enumerate((130.0, 180.0, 240.0))])
    got = tts.evaluate_ids(seqs, rec, rec_lens, "spk_c", return_path=True)
    pcms, lens = by_hand(tts, seqs, "spk_c")
    n = np.array([k * HOP for k in lens])
    synth = np.zeros((3, n.max()), np.int16)
    for i, (p, k) in enumerate(zip(pcms, n)):
        synth[i, :k] = p[:k]
    want = cmplib.compare_audio(rec, rec_lens, synth, n, SR, HOP, return_path=True)
    assert bitwise(got, want)
    for r, k, m in zip(got, rec_lens // HOP, lens):
        assert r["status"] == 0 and max(k, m) <= r["n_path"] <= k + m - 1 and r["mcd_db"] > 0 and r["mel_l1"] > 0
        assert tuple(r["path"][0]) == (0, 0) and tuple(r["path"][-1]) == (k - 1, m - 1)
    # a band, the frame-synchronous mode and the text entry go the same way
    assert bitwise(tts.evaluate_ids(seqs, rec, rec_lens, "spk_c", mode="sync"), cmplib.compare_audio(rec, rec_lens, synth, n, SR, HOP, mode="sync"))
    assert bitwise(tts.evaluate_ids(seqs, rec, rec_lens, "spk_c", band=8), cmplib.compare_audio(rec, rec_lens, synth, n, SR, HOP, band=8))
    texts = ["xin chao", "viet nam"]
    assert bitwise(tts.evaluate(texts, rec[:2], rec_lens[:2], "spk_b"), tts.evaluate_ids([tts.text_to_sequence(t) for t in texts], rec[:2], rec_lens[:2], "spk_b"))
    # behind wav_rate: the recordings at 44.1 kHz are converted on the device first
    from e2e_tts_amd import resample as rs
    up = rs.Resampler(SR, 44100)
    u = up.forward(rec, n_valid=rec_lens, want=("pcm",))
    down = rs.Resampler(44100, SR)
    d = down.forward(u["pcm"], n_valid=u["n_out"], want=("wav",))
    assert bitwise(tts.evaluate_ids(seqs, u["pcm"], u["n_out"], "spk_c", wav_rate=44100), cmplib.compare_audio(d["wav"], d["n_out"], synth, n, SR, HOP))
    up.close()
    down.close()
    with pytest.raises(ValueError, match="recordings for"):
        tts.evaluate_ids(seqs, rec[:2], rec_lens[:2], "spk_c")


def test_forward_audio_mel_post_against_the_recording_in_sync_mode():
    """What forward_audio's docstring describes: the teacher-forced mel_post and the recording's own mel lie on one frame grid and are
    compared without a search.  mel_l1 is the mean absolute difference of the two mels over each utterance's frames."""
    from test_gpu_f0_api import model
    M = model()
    g, m, pcm, nv = M["g"], M["m"], M["pcm"], M["nv"]
    out, _ = m.forward_audio(g["speakers"], g["ids"], g["txt_lens"], pcm, nv)
    mel_post, mel_lens = out[1], out[7]
    fe, trk, ml = m.recording_features(pcm, nv)
    assert np.array_equal(ml, mel_lens.cpu().numpy()) and trk is not None
    rec_mel = fe.forward(pcm, nv)["mel"]
    c = cmplib.Comparator(int(g["n_mel"]))
    c.set_a(fe, ml, trk)
    c.set_b(mel_post, mel_lens)
    res = c.run(mode="sync", return_path=True)
    post = mel_post.cpu().numpy().astype(np.float64)
    for b, r in enumerate(res):
        n = int(ml[b])
        want = np.abs(rec_mel[b, :n].astype(np.float64) - post[b, :n]).mean()
        assert r["n_path"] == n and np.array_equal(r["path"][:, 0], np.arange(n)) and np.array_equal(r["path"][:, 1], np.arange(n))
        assert abs(r["mel_l1"] - want) <= 1e-12 * want and r["mcd_db"] > 0 and np.isnan(r["f0_rmse_hz"])   # side B has no f0
    c.set_b(fe, ml, trk)   # the recording against itself
    assert all(r["mcd_db"] == 0.0 and r["mel_l1"] == 0.0 for r in c.run(mode="sync"))
    c.close()
