"""GPU parity (-m gpu) of the Fastformer encoder / decoder blocks (building_block.block_type "fastformer", csrc/fastformer.hip +
engine_acoustic.hip: fastformer_stack) against the fixtures tools/make_fastformer_goldens.py wrote from the reference's own run, and against the
numpy restatement tests/fastformer_ref.py on geometries no fixture has.

Bars: those tests/test_gpu_parity.py holds the Conformer fixtures to -- discrete outputs exact, taps / predictions / mel mean-L1 < 1e-5 on
the tiny model, mel and mel_post < 1e-4 at full size.  The full-size taps, for which that file has no bar, are held to twice the
reference's own fp32-vs-float64 distance on the fixture (`f64_*`, written by the golden tool: the -10000 the reference adds to every valid
position's logit rounds it to a 2^-10 grid, so two fp32 evaluations differ by single rounding steps; tests/test_fastformer_host.py)."""
import numpy as np
import pytest

from conftest import load_golden
from e2e_tts_amd import config as cfgmod, synth_weights as sw
from fastformer_ref import FastformerOracle, fastformer_config

pytestmark = pytest.mark.gpu

MEL_L1 = 1e-4
WAV_L1 = 1e-4
TINY = ("tiny_ff_b3", "tiny_ff_b1", "tiny_ff_long")
WANT = ("dur", "mel_lens", "pitch_idx", "energy_idx", "log_d", "pitch_pred", "energy_pred")

_ENGINES = {}


def setup_for(g, name):
    """(config, acoustic state, vocoder state, engine) of a fixture; one engine per model size (the fixtures share seeds)."""
    from e2e_tts_amd.runtime import engine_from_states
    tiny = name.startswith("tiny")
    key = (tiny, str(g["mode"]), tuple(int(x) for x in g["weight_seeds"]))
    if key not in _ENGINES:
        cfg = fastformer_config(cfgmod.tiny_config() if tiny else cfgmod.default_config())
        ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=key[2][0], mode=key[1])
        voc = sw.make_vocoder_state(cfg, seed=key[2][1])
        _ENGINES[key] = (cfg, ac, voc, engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, voc, device=0))
    return _ENGINES[key]


def mean_l1(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def strided(g, k, x):
    return x[:, ::int(g[k + "_stride"])] if k + "_stride" in g else x


def run_acoustic(eng, g, vocoder="fp32", decoder="fp32"):
    eng.set_precision(vocoder, decoder)
    d, p, e = (float(x) for x in g["controls"])
    r = eng.acoustic(g["ids"], g["lens"], np.array([int(g["speaker"])], np.int64), d, p, e, want=WANT)
    mel, mel_post = eng.fetch_mel(r["B"], r["T"])
    return r, mel, mel_post


def check_discrete(r, g):
    for k in ("dur", "mel_lens", "pitch_idx", "energy_idx"):
        np.testing.assert_array_equal(r[k], g[k])


@pytest.mark.parametrize("name", TINY)
def test_tiny_fixture_full_trace_fp32(name):
    g = load_golden(name)
    cfg, ac, voc, eng = setup_for(g, name)
    B, L = g["ids"].shape
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    r, mel, mel_post = run_acoustic(eng, g)
    got = dict(log_d=r["log_d"], pitch_pred=r["pitch_pred"], energy_pred=r["energy_pred"], enc_out=eng.fetch_tap("enc_out", (B, L, H)),
               dec_out=eng.fetch_tap("dec_out", (B, r["T"], H)), mel=mel, mel_post=mel_post)
    for k, v in got.items():
        print(f"{name} fp32 {k}: mean-L1 {mean_l1(v, g[k]):.3e}" + (f" (reference fp32 vs float64 {float(g['f64_' + k]):.3e})" if "f64_" + k in g else ""))
    check_discrete(r, g)
    assert mel.shape == g["mel"].shape
    for k, v in got.items():
        assert mean_l1(v, g[k]) < 1e-5, (name, k, mean_l1(v, g[k]))
    wav, pcm = eng.vocoder(None, r["B"], r["T"], wav=True, pcm=True)
    assert mean_l1(wav, g["wav"]) < WAV_L1 / 10
    close = np.abs(pcm.astype(np.int32) - (g["wav"] * 32768.0).astype(np.int16).astype(np.int32)) <= 1
    assert close.mean() >= 0.999


def test_full_size_fixture_fp32():
    """192 heads of size 2, B = 2 (230 and 41 phonemes), T = 1095: the split-N pooling with 69 row runs per utterance."""
    name = "full_ff_b2"
    g = load_golden(name)
    cfg, ac, voc, eng = setup_for(g, name)
    B, L = g["ids"].shape
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    r, mel, mel_post = run_acoustic(eng, g)
    got = dict(log_d=r["log_d"], enc_out=eng.fetch_tap("enc_out", (B, L, H)), dec_out=eng.fetch_tap("dec_out", (B, r["T"], H)), mel=mel,
               mel_post=mel_post)
    err = {k: mean_l1(strided(g, k, v), g[k]) for k, v in got.items()}
    for k in got:
        print(f"{name} fp32 {k}: mean-L1 {err[k]:.3e} (reference fp32 vs float64 {float(g['f64_' + k]):.3e})")
    check_discrete(r, g)
    assert strided(g, "mel", mel).shape == g["mel"].shape
    assert err["mel"] < MEL_L1 and err["mel_post"] < MEL_L1, err
    for k in ("enc_out", "dec_out", "log_d"):
        assert err[k] < 2.0 * float(g["f64_" + k]), (k, err[k])


@pytest.mark.parametrize("name", ["tiny_ff_b3", "full_ff_b2"])
def test_decoder_bf16x3(name):
    """Split-precision decoder GEMMs (q | k, transform, FFN); logits, shift, softmax and pooling stay fp32."""
    g = load_golden(name)
    cfg, ac, voc, eng = setup_for(g, name)
    r, mel, mel_post = run_acoustic(eng, g, "bf16x3", "bf16x3")
    err = mean_l1(strided(g, "mel_post", mel_post), g["mel_post"])
    print(f"{name} bf16x3 decoder: mel_post mean-L1 {err:.3e}")
    check_discrete(r, g)
    assert err < MEL_L1, err
    eng.set_precision("fp32", "fp32")


def test_two_calls_are_bit_identical_with_the_sequence_split_over_workgroups():
    """B = 1, T >= 768: the pooling runs in T / 16 workgroups per utterance whose partial (max, sum, weighted sum) triples a second kernel
    merges in row order -- no atomics, so nothing depends on the order the workgroups finish in."""
    g = load_golden("tiny_ff_b1")
    cfg, ac, voc, eng = setup_for(g, "tiny_ff_b1")
    eng.set_precision("fp32", "fp32")
    rng = np.random.Generator(np.random.PCG64(99))
    ids = rng.integers(4, 131, size=(1, 200)).astype(np.int64)
    lens = np.array([200], np.int64)
    spk = np.array([1], np.int64)
    outs = []
    for _ in range(3):
        r = eng.acoustic(ids, lens, spk, want=("mel_lens",))
        assert r["T"] >= 768, r["T"]
        outs.append(eng.fetch_mel(1, r["T"])[1].copy())
        eng.poison_workspace()
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    assert np.isfinite(outs[0]).all()


def test_ragged_synthesize_is_bit_identical_on_valid_samples():
    """Nothing of these blocks is skipped in a ragged batch (every padded row takes part in the pooling); postnet and vocoder keep their
    ragged limits.  The poison between the calls shows that no valid sample reads a row the ragged call left out."""
    g = load_golden("tiny_ff_b3")
    cfg, ac, voc, eng = setup_for(g, "tiny_ff_b3")
    d, p, e = (float(x) for x in g["controls"])
    spk = np.array([int(g["speaker"])], np.int64)
    hop = cfg["audio"]["stft"]["hop_length"]
    try:
        for prec in ("fp32", "bf16x3"):
            eng.set_precision(prec, "fp32")
            eng.set_ragged(False)
            full, mel_lens, T = eng.synthesize(g["ids"], g["lens"], spk, d, p, e)
            eng.set_ragged(True)
            eng.poison_workspace()
            rag, mel_lens2, T2 = eng.synthesize(g["ids"], g["lens"], spk, d, p, e)
            assert T == T2
            np.testing.assert_array_equal(mel_lens, g["mel_lens"])
            np.testing.assert_array_equal(mel_lens2, g["mel_lens"])
            for b, n in enumerate(mel_lens * hop):
                np.testing.assert_array_equal(rag[b, :n], full[b, :n])
            ref_pcm = (g["wav"] * 32768.0).astype(np.int16)
            ok = [np.abs(rag[b, :n].astype(np.int32) - ref_pcm[b, :n].astype(np.int32)) <= 1 for b, n in enumerate(mel_lens * hop)]
            assert np.concatenate(ok).mean() >= 0.999
    finally:
        eng.set_ragged(True)
        eng.set_precision("fp32", "fp32")


def _geometry(which):
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    if which == "heads":      # decoder_head != encoder_head: 64 heads of size 1 in the encoder, 8 heads of size 8 in the decoder
        cfg = fastformer_config(cfg, encoder_head=1, decoder_head=8, conv_filter_size=100, conv_kernel_size=(5, 1))
        cfg["models"]["fastspeech2"]["encoder_layers"], cfg["models"]["fastspeech2"]["decoder_layers"] = 1, 3
    else:                     # hidden 128, head size 4: 32 heads
        fs["encoder_hidden"] = fs["decoder_hidden"] = 128
        cfg = fastformer_config(cfg, encoder_head=4, decoder_head=4, conv_filter_size=136, conv_kernel_size=(3, 1))
    return cfg


@pytest.mark.parametrize("which,lens", [("heads", [29, 7, 18]), ("h128", [33, 33, 1, 12])])
def test_other_geometries_match_the_restatement(which, lens):
    from e2e_tts_amd.runtime import engine_from_states
    from oracle import ref_numpy as orc
    from oracle.make_goldens import search_ids
    cfg = _geometry(which)
    stats = cfgmod.DEFAULT_STATS
    seed = 11 if which == "heads" else 12
    ac = sw.make_acoustic_state(cfg, stats, 4, seed=700 + seed, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=800 + seed)
    o = FastformerOracle(ac, cfg, stats)
    lens = np.array(lens, np.int64)
    spk_id = seed % 4
    _, ids = search_ids(o, [int(x) for x in lens], spk_id, stats, (1.0, 1.0, 1.0), 2e-3, 40, 5000 + 100 * seed, False)
    spk = np.array([spk_id], np.int64)
    (omel, omel_post, odur), omel_lens = o.inference(spk, ids, lens)
    owav = orc.VocoderOracle(voc, cfg).forward(omel_post.transpose(0, 2, 1))[:, 0]
    hop = cfg["audio"]["stft"]["hop_length"]
    eng = engine_from_states(cfg, stats, ac, voc)
    try:
        for prec in ("fp32", "bf16x3"):
            eng.set_precision(prec)
            r = eng.acoustic(ids, lens, spk, want=("dur", "mel_lens", "pitch_idx", "energy_idx"))
            mel, mel_post = eng.fetch_mel(r["B"], r["T"])
            print(f"{which} {prec}: mel_post mean-L1 {mean_l1(mel_post, omel_post):.3e}")
            np.testing.assert_array_equal(r["dur"], odur)
            np.testing.assert_array_equal(r["mel_lens"], omel_lens)
            np.testing.assert_array_equal(r["pitch_idx"], o.trace["pitch_idx"])
            np.testing.assert_array_equal(r["energy_idx"], o.trace["energy_idx"])
            assert mean_l1(mel_post, omel_post) < MEL_L1, (which, prec, mean_l1(mel_post, omel_post))
            wav, _ = eng.vocoder(None, r["B"], r["T"])
            assert mean_l1(wav, owav) < WAV_L1, (which, prec, mean_l1(wav, owav))
            eng.set_ragged(False)
            full, ml, T = eng.synthesize(ids, lens, spk)
            eng.set_ragged(True)
            eng.poison_workspace()
            rag, ml2, T2 = eng.synthesize(ids, lens, spk)
            assert T == T2 and np.array_equal(ml, ml2) and np.array_equal(ml, omel_lens)
            for b, n in enumerate(ml * hop):
                np.testing.assert_array_equal(rag[b, :n], full[b, :n])
    finally:
        eng.close()
