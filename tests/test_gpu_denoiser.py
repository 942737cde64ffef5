"""GPU tests (-m gpu) of the vocoder-bias denoiser (csrc/denoiser.hip, engine_denoise.hip: denoise_impl; include/e2etts.h: e2etts_denoiser_*,
e2etts_denoise, e2etts_set_denoise) against tests/golden/denoiser.npz, which tools/make_denoiser_goldens.py wrote from the reference's
own module (V/denoiser.py) run on every row alone.

Bars.  Against the reference's float64 run, on valid samples: mean-L1 <= 4 x dref and max-abs <= 8 x dmax, dref / dmax being the
reference's own fp32-vs-float64 distances stored in the fixture (the factors cover two chained exact-fp32 transforms summed in MFMA order, in
chains of 1024 and 1056 terms, where the CPU sums in blocks).  int16 within 1 LSB of trunc(reference fp32 x 32768) on >= 99.9 % of the valid samples (the
project's PCM gate).  Samples at or past a row's length exactly 0.  Calibration: sum |bias - reference bias| <= 1e-4 x sum |reference bias|
-- the project's wav gate (mean-L1 1e-4 on a waveform of order 1; the transform is linear, so the gate scales with the spectrum's norm).
Measured figures are printed before each assertion (tools/denoiser_bench.py and profiles/denoiser/README.md keep them).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from e2e_tts_amd import config as cfgmod, denoiser as dn, synth_weights as sw
from e2e_tts_amd._lib import E_INVAL, E_OK, E_STATE, _addr

pytestmark = pytest.mark.gpu

CANARY_F, CANARY_I, MARGIN = np.float32(-7.25e9), np.int16(-21555), 1024
_STATE = {}


def new_engine():
    from e2e_tts_amd.runtime import engine_from_states
    if "weights" not in _STATE:
        cfg = cfgmod.tiny_config()
        _STATE["weights"] = (cfg, sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=1234, mode="varied"), sw.make_vocoder_state(cfg, seed=4321))
    cfg, ac, voc = _STATE["weights"]
    return engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, voc, device=0)


@pytest.fixture(scope="module")
def gold():
    return load_golden("denoiser")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def load_geometry(eng, N, V):
    key = (N, V)
    if key not in _STATE:
        _STATE[key] = dn.stft_bases(N, N // V, N)
    fwd, inv, win_sq = _STATE[key]
    eng.denoiser_load(fwd, inv, N, N // V, dn.engine_window(win_sq, N, N, "hann"))
    return N // V


def guarded(shape, dtype, canary):
    """An output buffer with canary margins on both sides: (whole, view)."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * MARGIN, canary, dtype)
    return whole, whole[MARGIN:MARGIN + n].reshape(shape)


def margins_intact(whole, canary):
    return bool((whole[:MARGIN] == canary).all() and (whole[-MARGIN:] == canary).all())


def run(eng, audio, n_valid, strength):
    """denoise into canary-guarded host buffers -> (wav, pcm); the margins are checked here (test 6)."""
    ww, w = guarded(audio.shape, np.float32, CANARY_F)
    pw, p = guarded(audio.shape, np.int16, CANARY_I)
    eng.denoise(np.ascontiguousarray(audio), None if n_valid is None else np.asarray(n_valid, np.int64), strength, out_wav=w, out_pcm=p)
    assert margins_intact(ww, CANARY_F) and margins_intact(pw, CANARY_I)
    assert not (w == CANARY_F).any()
    return w.copy(), p.copy()


def valid_dist(a, b, n_valid, rows=None):
    rows = range(len(n_valid)) if rows is None else rows
    d = np.concatenate([np.abs(a[i, :n_valid[i]].astype(np.float64) - b[i, :n_valid[i]].astype(np.float64)) for i in rows])
    return float(d.mean()), float(d.max())


def pcm_close(pcm, ref32, n_valid):
    want = np.trunc(ref32.astype(np.float32) * np.float32(32768.0)).clip(-32768, 32767).astype(np.int32)
    ok = np.concatenate([np.abs(pcm[i, :nb].astype(np.int32) - want[i, :nb]) <= 1 for i, nb in enumerate(n_valid)])
    return float(ok.mean())


@pytest.mark.parametrize("tag", ("a", "b"))
@pytest.mark.parametrize("si", (0, 1))
def test_denoise_matches_the_reference_row_by_row(eng, gold, tag, si):
    N, V = (int(x) for x in gold[f"{tag}_geometry"])
    load_geometry(eng, N, V)
    eng.denoiser_set_bias(gold[f"{tag}_bias"])
    nv, s = [int(x) for x in gold[f"{tag}_n_valid"]], float(gold[f"{tag}_strengths"][si])
    wav, pcm = run(eng, gold[f"{tag}_audio"], nv, s)
    o32, o64 = gold[f"{tag}_out32_s{si}"], gold[f"{tag}_out64_s{si}"]
    dref, dmax = float(gold[f"{tag}_dref"][si]), float(gold[f"{tag}_dmax"][si])
    mean, mx = valid_dist(wav, o64, nv)
    frac = pcm_close(pcm, o32, nv)
    print(f"denoiser ({N}, {V}) strength {s}: vs reference float64 mean-L1 {mean:.3e} (reference fp32 {dref:.3e}, bar {4 * dref:.3e}) "
          f"max {mx:.3e} (reference {dmax:.3e}, bar {8 * dmax:.3e}); vs reference fp32 mean-L1 {valid_dist(wav, o32, nv)[0]:.3e}; "
          f"int16 within 1 LSB {100 * frac:.3f} %")
    assert mean <= 4 * dref and mx <= 8 * dmax
    assert frac >= 0.999
    for b, nb in enumerate(nv):
        assert not wav[b, nb:].any() and not pcm[b, nb:].any()
    if tag == "a":   # the shortest legal row (768 samples: both reflections fall into the same frames), against its own reference distances
        m2, x2 = valid_dist(wav, o64, nv, rows=[2])
        r2, rx2 = valid_dist(o32, o64, nv, rows=[2])
        print(f"    768-sample row: mean-L1 {m2:.3e} (reference fp32 {r2:.3e}) max {x2:.3e} ({rx2:.3e})")
        assert nv[2] == 768 and m2 <= 4 * r2 and x2 <= 8 * rx2


def test_rows_at_or_under_half_a_filter_pass_through_bit_equal(eng, gold):
    load_geometry(eng, 1024, 4)
    eng.denoiser_set_bias(gold["a_bias"])
    audio = gold["a_audio"][:, :2048].copy()
    nv = [2048, 512, 256]
    wav, pcm = run(eng, audio, nv, 0.1)
    for b in (1, 2):
        np.testing.assert_array_equal(wav[b, :nv[b]], audio[b, :nv[b]])
        np.testing.assert_array_equal(pcm[b, :nv[b]], np.trunc(audio[b, :nv[b]] * np.float32(32768.0)).astype(np.int16))
        assert not wav[b, nv[b]:].any() and not pcm[b, nv[b]:].any()
    alone, _ = run(eng, audio[:1], None, 0.1)
    np.testing.assert_array_equal(wav[0], alone[0])
    assert np.abs(wav[0] - audio[0]).mean() > 1e-4   # and the long row was denoised
    # a batch of nothing but short rows: no transform at all
    w2, _ = run(eng, audio[1:], [512, 0], 0.1)
    np.testing.assert_array_equal(w2[0, :512], audio[1, :512])
    assert not w2[0, 512:].any() and not w2[1].any()


@pytest.mark.parametrize("tag", ("a", "b"))
def test_a_row_of_a_ragged_batch_equals_the_utterance_alone(eng, gold, tag):
    N, V = (int(x) for x in gold[f"{tag}_geometry"])
    hop = load_geometry(eng, N, V)
    eng.denoiser_set_bias(gold[f"{tag}_bias"])
    audio = gold[f"{tag}_audio"]
    nv = [int(x) for x in gold[f"{tag}_n_valid"]]
    if tag == "b":
        nv = [2048, 5 * hop]   # the fixture's rows are equally long: cut one
    wav, pcm = run(eng, audio, nv, 0.1)
    for b, nb in enumerate(nv):
        w1, p1 = run(eng, audio[b:b + 1, :nb], None, 0.1)
        np.testing.assert_array_equal(wav[b, :nb], w1[0])
        np.testing.assert_array_equal(pcm[b, :nb], p1[0])


def test_calibration_on_the_engines_vocoder(eng, gold):
    import torch
    load_geometry(eng, 1024, 4)
    # something resident first: calibration must leave it alone
    mel = gold["c_mel"]
    wav0, pcm0 = eng.vocoder(mel, mel.shape[0], mel.shape[2], wav=True, pcm=True)
    bias = eng.denoiser_calibrate(None, 88)
    ref = gold["c_bias_spec"].astype(np.float64)
    rel = float(np.abs(bias.astype(np.float64) - ref).sum() / np.abs(ref).sum())
    print(f"calibrate(None, 88): relative L1 of the bias spectrum vs the reference's {rel:.3e} (bar 1e-4); max |d| {np.abs(bias - ref).max():.3e}")
    assert bias.shape == ref.shape and rel <= 1e-4
    np.testing.assert_array_equal(eng.fetch_wav(mel.shape[0], mel.shape[2]), wav0)
    assert valid_dist(wav0, gold["c_audio"], [wav0.shape[1]] * 2)[0] <= 1e-5   # the engine's vocoder makes the fixture's audio of that mel
    s = float(gold["c_strength"])
    # denoise of the RESIDENT wav (NULL input) is denoise of that wav handed in, and leaves it resident
    eng.denoiser_set_bias(bias)
    w_res, _ = eng.denoise(None, None, s, B=2, n=wav0.shape[1])
    np.testing.assert_array_equal(w_res, run(eng, wav0, None, s)[0])
    np.testing.assert_array_equal(eng.fetch_wav(mel.shape[0], mel.shape[2]), wav0)
    # device buffers with margins (torch tensors): the copies stay inside them
    whole = torch.full((2 * wav0.shape[1] + 2 * MARGIN,), float(CANARY_F), dtype=torch.float32, device="cuda:0")
    view = whole[MARGIN:MARGIN + 2 * wav0.shape[1]].view(2, -1)
    eng.denoise(torch.from_numpy(wav0).to("cuda:0"), None, s, out_wav=view)
    torch.cuda.synchronize()
    assert bool((whole[:MARGIN] == float(CANARY_F)).all()) and bool((whole[-MARGIN:] == float(CANARY_F)).all())
    np.testing.assert_array_equal(view.cpu().numpy(), w_res)


def test_vocoder_audio_with_the_references_bias(eng, gold):
    """Fixture (c)'s vocoder audio, denoised with the reference's own bias spectrum, against the reference's float64 run at the factors
    of (a) and (b): 4 x its fp32-vs-float64 mean-L1, 8 x its max.

    This audio (a random-weight vocoder's output) carries a constant offset, and the reference's own distance on it is half that of (a)
    and (b), so it is the hardest of the three for a GEMM that sums in one chain.  With the inverse transform as ONE KW = n_overlap
    convolution (a chain of 4 224 terms per sample) the MI355X measured mean-L1 5.934e-08 against the bar of 5.214e-08 and max 7.888e-07
    against 6.009e-07: not met.  The inverse now runs as one accumulated launch per tap (engine_denoise.hip: denoise_impl); measured in that
    form: 2.595e-08 / 2.448e-07."""
    load_geometry(eng, 1024, 4)
    eng.denoiser_set_bias(gold["c_bias_spec"])
    nv = [gold["c_audio"].shape[1]] * 2
    w_ref, p_ref = run(eng, gold["c_audio"], nv, float(gold["c_strength"]))
    mean, mx = valid_dist(w_ref, gold["c_out64"], nv)
    print(f"vocoder audio, reference's bias: mean-L1 {mean:.3e} (reference fp32 {float(gold['c_dref']):.3e}, bar {4 * float(gold['c_dref']):.3e}) "
          f"max {mx:.3e} ({float(gold['c_dmax']):.3e}, bar {8 * float(gold['c_dmax']):.3e})")
    assert pcm_close(p_ref, gold["c_out32"], nv) >= 0.999
    assert mean <= 4 * float(gold["c_dref"]) and mx <= 8 * float(gold["c_dmax"])


def test_set_denoise_in_synthesize_is_denoise_of_the_resident_wav(eng):
    g = load_golden("tiny_b3")
    ids, lens, spk = g["ids"], g["lens"], np.array([int(g["speaker"])], np.int64)
    load_geometry(eng, 1024, 4)
    eng.denoiser_calibrate(None, 88)
    hop = eng.dims.hop_length
    try:
        eng.set_denoise(0.1)
        pcm_d, mel_lens, T = eng.synthesize(ids, lens, spk)
        wav = eng.fetch_wav(len(lens), T)
        eng.set_denoise(0.0)
        pcm_0, mel_lens0, T0 = eng.synthesize(ids, lens, spk)
    finally:
        eng.set_denoise(0.0)
    np.testing.assert_array_equal(mel_lens, g["mel_lens"])
    assert T == T0 and (mel_lens == mel_lens0).all()
    nv = [int(m) * hop for m in mel_lens]
    differs = 0
    for b, nb in enumerate(nv):
        _, p1 = run(eng, wav[b:b + 1, :nb], None, 0.1)
        np.testing.assert_array_equal(pcm_d[b, :nb], p1[0])
        assert not pcm_d[b, nb:].any()
        differs += int((pcm_d[b, :nb] != pcm_0[b, :nb]).sum())
    _, pb = run(eng, wav, nv, 0.1)
    np.testing.assert_array_equal(pcm_d, pb)
    assert differs > 0
    # strength 0 is the path of an engine that never saw a denoiser.  Valid samples only: in ragged mode (the default) what lies past a row's
    # length in the padded PCM is whatever the workspace held -- unspecified (include/e2etts.h: e2etts_set_ragged), and the two engines' histories differ
    plain = new_engine()
    pcm_p, mel_lens_p, T_p = plain.synthesize(ids, lens, spk)
    assert T_p == T
    for b, nb in enumerate(nv):
        np.testing.assert_array_equal(pcm_0[b, :nb], pcm_p[b, :nb])
    plain.close()


def test_bad_arguments_return_their_codes(gold):
    e = new_engine()
    lib, h = e.lib, e._h
    x = np.zeros((1, 2048), np.float32)
    out = np.zeros((1, 2048), np.float32)
    nv = np.array([2048], np.int64)

    def denoise(inp=x, n_valid=nv, B=1, n=2048):
        return lib.e2etts_denoise(h, _addr(inp), _addr(n_valid), B, n, 0.1, _addr(out), None)

    fwd, inv, _ = dn.stft_bases(1024, 256, 1024)
    bias = np.ascontiguousarray(gold["a_bias"])
    assert denoise() == E_STATE and b"bases" in lib.e2etts_last_error(h)                      # no bases loaded
    assert lib.e2etts_set_denoise(h, 0.1) == E_STATE
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), bias.size) == E_STATE
    assert lib.e2etts_denoiser_calibrate(h, None, 88, None) == E_STATE
    for N, hop in ((1024, 1024), (1024, 64), (1000, 250), (768, 256), (4096, 2048)):       # unsupported geometries, numbers in the message
        assert lib.e2etts_denoiser_load(h, _addr(fwd), _addr(inv), None, N, hop) == E_INVAL
        assert str(N).encode() in lib.e2etts_last_error(h) and str(hop).encode() in lib.e2etts_last_error(h)
    assert denoise() == E_STATE                                                              # a refused load loads nothing
    assert lib.e2etts_denoiser_load(h, _addr(fwd), _addr(inv), None, 1024, 256) == E_OK
    assert denoise() == E_STATE and b"bias" in lib.e2etts_last_error(h)                       # no bias set
    assert lib.e2etts_set_denoise(h, 0.1) == E_STATE
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), bias.size - 1) == E_INVAL
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), bias.size) == E_OK
    for bad in (2047, 100, 2304, -256):                                                       # n_b % hop != 0, n_b > n, n_b < 0
        assert denoise(n_valid=np.array([bad], np.int64)) == E_INVAL
    assert denoise(inp=None) == E_STATE and b"resident" in lib.e2etts_last_error(h)          # NULL input, nothing resident
    assert lib.e2etts_denoise(h, _addr(x), _addr(nv), 1, 2048, 0.1, None, None) == E_INVAL
    assert lib.e2etts_denoiser_calibrate(h, None, 1, None) == E_INVAL                        # 256 samples: under half a filter
    assert lib.e2etts_set_denoise(h, C.c_float(-1.0)) == E_INVAL
    # ... and the engine is as usable as before: nothing was launched on bad arguments
    assert denoise() == E_OK and not out.any()
    with pytest.raises(ValueError):
        e.denoise(x, np.array([100], np.int64), 0.1)
    # a row too long for 32-bit offsets into its spectrum is refused by the entry point itself, with the limit in the message
    assert lib.e2etts_denoise(h, _addr(x), None, 1, 1 << 29, 0.1, _addr(out), None) == E_INVAL and b"2 GiB" in lib.e2etts_last_error(h)
    assert denoise() == E_OK
    e.close()
    fresh = new_engine()
    with pytest.raises(RuntimeError):
        fresh.denoise(x, nv, 0.1)
    fresh.close()


def test_calibration_leaves_the_istft_vocoders_resident_results_alone():
    """The iSTFT tail keeps tap buffers besides wav and PCM: a calibration pass works in buffers of its own, so all three resident results
    read the same bytes after it as before, and a second identical calibration allocates nothing."""
    from e2e_tts_amd import packer
    from e2e_tts_amd._lib import Engine
    cfg = cfgmod.tiny_config()
    dims = cfgmod.dims_from_config(cfg, cfgmod.DEFAULT_STATS, 4, vocoder="istft")
    eng = Engine(dims, 0)
    eng.load_weights(packer.pack(dims, sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=21, mode="varied"),
                                 sw.make_vocoder_state(cfg, seed=22, vocoder="istft")))
    N = 1024
    dhop = load_geometry(eng, N, 4)
    B, T = 2, 8
    mel = np.random.Generator(np.random.PCG64(31)).standard_normal((B, T, dims.n_mel)).astype(np.float32)
    up = dims.hop_length // dims.voc_istft_hop
    tap_shape = (B, T * up + 1, dims.voc_istft_nfft + 2)

    def resident():
        pcm = np.empty((B, T * dims.hop_length), np.int16)
        assert eng.lib.e2etts_fetch_pcm(eng._h, _addr(pcm), pcm.size) == E_OK
        return eng.fetch_wav(B, T), pcm, eng.fetch_tap("istft_spec_phase", tap_shape)

    wav0, pcm0 = eng.vocoder(mel, B, T, channels_first=False, wav=True, pcm=True)
    before = resident()
    np.testing.assert_array_equal(before[0], wav0)
    np.testing.assert_array_equal(before[1], pcm0)
    assert np.abs(before[2]).max() > 0
    # the smallest frame count the call accepts: a multiple of the denoiser hop in samples, above filter_length / 2
    T_c = next(t for t in range(1, N) if (t * dims.hop_length) % dhop == 0 and t * dims.hop_length > N // 2)
    assert eng.lib.e2etts_denoiser_calibrate(eng._h, None, T_c - 1, None) == E_INVAL
    eng.denoiser_calibrate(None, T_c)
    for a, b in zip(resident(), before):
        assert a.tobytes() == b.tobytes()
    held = eng.device_bytes()
    eng.denoiser_calibrate(None, T_c)
    assert eng.device_bytes() == held
    for a, b in zip(resident(), before):
        assert a.tobytes() == b.tobytes()
    eng.close()
