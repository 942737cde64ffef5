"""The corpus statistics through the public interfaces: CorpusStats.add_recordings against add of the arrays fetched from the mel front-end
and the pitch tracker, UnsupervisedFastSpeech2.forward_audio(e_targets="extract") against the same target made by the numpy restatement
and handed in, bit for bit, models.build_stats and TTS.build_stats."""
import json

import numpy as np
import pytest

import stats_ref as sr
from e2e_tts_amd import config as cfgmod, stats as stlib, synth_weights as sw
from test_gpu_f0_api import model

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).tobytes()


def fetched(m, pcm, nv):
    """(energy [B, T], f0 [B, T], mel_lens) of the recordings, fetched from the front-end and the tracker to the host"""
    fe = m._default_stft().frontend
    r = fe.forward(pcm, nv, want=("energy",))
    trk = m.recording_features(pcm, nv)[1]
    t = trk.forward(pcm, nv)
    assert t["T"] == r["T"]
    return np.asarray(r["energy"], np.float32), np.asarray(t["f0"], np.float32), np.asarray(r["mel_lens"], np.int64)


def test_add_recordings_equals_add_of_the_fetched_arrays():
    M = model()
    m, pcm, nv = M["m"], M["pcm"], M["nv"]
    assert pcm.shape[0] == 3
    energy, f0, ml = fetched(m, pcm, nv)
    assert (f0 != 0).any() and (f0 == 0).any()
    a, b = stlib.CorpusStats(), stlib.CorpusStats()
    try:
        got_ml = a.add_recordings(m, pcm, nv)
        assert np.array_equal(got_ml, ml)
        b.add(energy=energy, lens=ml)
        b.add(f0=f0, lens=ml)
        assert bits(a.blocks()) == bits(b.blocks())
        res = a.result()
        assert set(res) == {"f0", "energy"} and res == b.result()
        # and that is the definition, on the host: the discrete figures exactly, the others under the bars
        ref = sr.corpus([{"energy": energy[i, :n], "f0": f0[i, :n]} for i, n in enumerate(ml)], kinds=("f0", "energy"))
        for k in ("f0", "energy"):
            assert sr.check_block(res[k], ref[k], ref["_bars"][k], k != "f0") == [], k
        blk = a.blocks()
        assert blk["n_kept"][stlib.ENERGY] == ref["energy"]["n_kept"] and blk["n_kept"][stlib.F0] == ref["f0"]["n_kept"]
        # batch by batch gives the same bits
        a.reset()
        a.add_recordings(m, pcm[:1], nv[:1])
        a.add_recordings(m, pcm[1:], nv[1:])
        assert bits(a.blocks()) == bits(b.blocks())
    finally:
        a.close()
        b.close()


def test_forward_audio_extracts_the_energy_target():
    import torch
    M = model()
    g, m, pcm, nv = M["g"], M["m"], M["pcm"], M["nv"]
    args = (g["speakers"], g["ids"], g["txt_lens"])
    energy, _, ml = fetched(m, pcm, nv)
    from e2e_tts_amd import models
    with pytest.raises(ValueError, match="stats\\['energy'\\]"):                        # the default stats carry no energy mean: refused before any launch
        m.forward_audio(*args, pcm, nv, e_targets="extract")
    st = models.build_stats(m, [(pcm, nv)])["energy"]                                  # the loop closed: the statistics of these recordings
    saved = m.stats
    m.stats = {**saved, "energy": {**saved["energy"], "mean": st["mean"], "std": st["std"]}}
    try:
        _extract_checks(m, args, pcm, nv, sr.normalize(energy, ml, st["mean"], st["std"]))
    finally:
        m.stats = saved


def _extract_checks(m, args, pcm, nv, target):
    import torch
    assert np.abs(target).max() > 0

    def same(a, b):
        (ma, pa, _, _, ea, *_), (_, ta) = a
        (mb, pb, _, _, eb, *_), (_, tb) = b
        return all(bits(x.cpu().numpy()) == bits(y.cpu().numpy()) for x, y in ((ma, mb), (pa, pb), (ea, eb), (ta, tb)))

    for step in (0, 10 ** 9):
        got = m.forward_audio(*args, pcm, nv, e_targets="extract", step=step)
        assert same(got, m.forward_audio(*args, pcm, nv, e_targets=target, step=step))
        assert same(got, m.forward_audio(*args, pcm, nv, e_targets=torch.from_numpy(target).cuda(), step=step))
    # with the pitch targets extracted too
    both = m.forward_audio(*args, pcm, nv, p_targets="extract", e_targets="extract")
    assert bits(both[1][1].cpu().numpy()) == bits(got[1][1].cpu().numpy()) and both[1][0] is not None
    # e_targets=None is what it was: the prediction is embedded, no target comes back; and the target matters
    a, b = m.forward_audio(*args, pcm, nv), m.forward_audio(*args, pcm, nv, e_targets=None)
    assert a[1][1] is None and b[1][1] is None and all(bits(x.cpu().numpy()) == bits(y.cpu().numpy()) for x, y in zip(a[0][:5], b[0][:5]))
    assert bits(a[0][1].cpu().numpy()) != bits(m.forward_audio(*args, pcm, nv, e_targets="extract")[0][1].cpu().numpy())
    with pytest.raises(ValueError, match="'extract'"):
        m.forward_audio(*args, pcm, nv, e_targets="rms")


def test_build_stats_through_the_mirrors(tmp_path_factory):
    from test_gpu_denoiser_api import write_checkpoints
    from e2e_tts_amd import models
    from e2e_tts_amd.api import TTS
    M = model()
    m, pcm, nv, g = M["m"], M["pcm"], M["nv"], M["g"]
    want = models.build_stats(m, [(pcm, nv)])
    assert want == models.build_stats(m, [(pcm[:2], nv[:2]), (pcm[2:], nv[2:])])
    cfg = cfgmod.tiny_config()
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=7, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=8)
    apath, vpath = write_checkpoints(tmp_path_factory.mktemp("ckpt"), cfg, ac, voc)
    tts = TTS(apath, vpath, max_len=60)
    got = tts.build_stats(pcm, nv, batch=2)
    assert set(got) == {"f0", "energy"} and set(got["energy"]) == {"max", "min", "mean", "std"} and set(got["f0"]) == {"mean", "std"}
    assert json.loads(json.dumps(got)) == got and all(isinstance(v, float) and np.isfinite(v) for blk in got.values() for v in blk.values())
    assert got == tts.build_stats(pcm, nv, batch=1) == tts.build_stats(pcm, nv)
    assert got["energy"]["min"] < 0 < got["energy"]["max"] and got["energy"]["std"] > 0 and got["f0"]["mean"] > 50
    fs = cfg["models"]["fastspeech2"]
    m2 = models.UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, got, device=0)        # a file without "pitch" serves a use_uv model
    assert m2.stats is got and stlib.bins(got)[0] is None and stlib.bins(got)[1].shape == (255,)
    with pytest.raises(ValueError, match="batch"):
        tts.build_stats(pcm, nv, batch=0)
