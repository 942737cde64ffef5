"""GPU tests (-m gpu) of the denoised vocoder stream (include/e2etts.h: e2etts_vocoder_stream_begin_denoised; engine_denoise.hip:
denoise_stream_impl; csrc/denoiser.hip: the stream forms of the pad and overlap-add passes).

The contract is bit equality: the concatenated pieces of a denoised stream are e2etts_denoise of the one-shot vocoder's waveform, as fp32
and as int16, for any chunking, in every precision, with two chunks in flight (assert_array_equal throughout).  One test holds the stream
to the reference's own output (fixture c of tests/golden/denoiser.npz) at the bars tests/test_gpu_denoiser.py holds the one-shot path to.
Every test calls the new entry.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from e2e_tts_amd import config as cfgmod, denoiser as dn, synth_weights as sw
from e2e_tts_amd._lib import E_INVAL, E_OK, E_STATE, _addr

pytestmark = pytest.mark.gpu

CANARY_F, CANARY_I, MARGIN = np.float32(-7.25e9), np.int16(-21555), 1024
B, T = 3, 96
CHUNKINGS = ([96], [1] * 96, [1, 7, 40, 3, 45], [50, 46])
_STATE = {}


def new_engine(seed=4321):
    from e2e_tts_amd.runtime import engine_from_states
    cfg = cfgmod.tiny_config()
    if "ac" not in _STATE:
        _STATE["ac"] = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=1234, mode="varied")
    return engine_from_states(cfg, cfgmod.DEFAULT_STATS, _STATE["ac"], sw.make_vocoder_state(cfg, seed=seed), device=0)


@pytest.fixture(scope="module")
def eng():
    e = new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def mel():
    return np.random.Generator(np.random.PCG64(2024)).standard_normal((B, T, 80)).astype(np.float32)


def load_geometry(eng, N, V, bias=None):
    """Bases of (N, V) and a bias: the given one, or a fixed positive random spectrum (large enough for the subtraction to bite)."""
    if (N, V) not in _STATE:
        _STATE[(N, V)] = dn.stft_bases(N, N // V, N)
    fwd, inv, win_sq = _STATE[(N, V)]
    assert eng.lib.e2etts_vocoder_stream_begin(eng._h, 1) >= 0   # abandons a denoised stream an earlier, failed test may have left open
    eng.denoiser_load(fwd, inv, N, N // V, dn.engine_window(win_sq, N, N, "hann"))
    if bias is None:
        bias = (np.abs(np.random.Generator(np.random.PCG64(N + V)).standard_normal(N // 2 + 1)) * 0.5).astype(np.float32)
    eng.denoiser_set_bias(np.ascontiguousarray(bias, dtype=np.float32))


def guarded(shape, dtype, canary):
    n = int(np.prod(shape))
    whole = np.full(n + 2 * MARGIN, canary, dtype)
    return whole, whole[MARGIN:MARGIN + n].reshape(shape)


def margins_intact(whole, canary):
    return bool((whole[:MARGIN] == canary).all() and (whole[-MARGIN:] == canary).all())


def begin(eng, nb, strength):
    d = C.c_int(-1)
    rc = eng.lib.e2etts_vocoder_stream_begin_denoised(eng._h, nb, C.c_float(strength), C.byref(d))
    return rc, d.value


def push(eng, chunk, last):
    n = C.c_int(-1)
    rc = eng.lib.e2etts_vocoder_stream_push(eng._h, _addr(chunk), int(chunk.shape[1]), int(last), C.byref(n))
    return rc, n.value


def fetch(eng, nb, n_emit):
    """The oldest unfetched chunk into canary-guarded buffers -> (wav, pcm)."""
    ns = n_emit * eng.dims.hop_length
    ww, w = guarded((nb, ns), np.float32, CANARY_F)
    pw, p = guarded((nb, ns), np.int16, CANARY_I)
    rc = eng.lib.e2etts_vocoder_stream_fetch(eng._h, _addr(w), _addr(p), w.size)
    assert rc == E_OK, eng.lib.e2etts_last_error(eng._h).decode()
    assert margins_intact(ww, CANARY_F) and margins_intact(pw, CANARY_I)
    assert not (w == CANARY_F).any()
    return w.copy(), p.copy()


def cut(mel, sizes):
    assert sum(sizes) == mel.shape[1]
    pos, out = 0, []
    for n in sizes:
        out.append(np.ascontiguousarray(mel[:, pos:pos + n]))
        pos += n
    return out


def stream(eng, mel, sizes, strength, between=None):
    """The raw ABI with two chunks in flight (push i + 1, then fetch i) -> (wav, pcm, halo, delay, [(frames pushed, frames emitted)])."""
    nb = mel.shape[0]
    halo, delay = begin(eng, nb, strength)
    assert halo >= 0, eng.lib.e2etts_last_error(eng._h).decode()
    got, waiting, lag, pushed, emitted = [], [], [], 0, 0
    chunks = cut(mel, sizes)
    for i, c in enumerate(chunks):
        rc, n = push(eng, c, i == len(chunks) - 1)
        assert rc == E_OK, eng.lib.e2etts_last_error(eng._h).decode()
        pushed += c.shape[1]
        emitted += n
        lag.append((pushed, emitted))
        if n > 0:
            waiting.append(n)
        if len(waiting) == 2:
            got.append(fetch(eng, nb, waiting.pop(0)))
        if between:
            between()
    while waiting:
        got.append(fetch(eng, nb, waiting.pop(0)))
    return np.concatenate([g[0] for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1), halo, delay, lag


def one_shot(eng, mel, strength):
    """e2etts_denoise of e2etts_vocoder of the whole mel -> (vocoder wav, vocoder pcm, denoised wav, denoised pcm)."""
    nb, t = mel.shape[0], mel.shape[1]
    wav, pcm = eng.vocoder(mel, nb, t, channels_first=False, pcm=True)
    w, p = eng.denoise(wav, None, strength, want_pcm=True)
    return wav, pcm, w, p


# 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
@pytest.mark.parametrize("N,V", ((1024, 4), (512, 2), (256, 4), (1024, 8)))
def test_stream_pieces_equal_one_shot_denoise_bit_for_bit(eng, mel, N, V, prec):
    eng.set_precision(prec)
    load_geometry(eng, N, V)
    hl = eng.dims.hop_length
    C_ = dn.stream_delay_frames(N, N // V, hl)
    for strength in (0.1, 0.0):
        voc, _, want, want_pcm = one_shot(eng, mel, strength)
        if strength:
            assert np.abs(want - voc).mean() > 1e-5   # the subtraction does something on this audio
        for sizes in CHUNKINGS:
            wav, pcm, halo, delay, lag = stream(eng, mel, sizes, strength)
            assert delay == C_
            np.testing.assert_array_equal(wav, want)
            np.testing.assert_array_equal(pcm, want_pcm)
            for pushed, emitted in lag[:-1]:   # until the last push, emitted frames lag pushed ones by halo + C
                assert emitted == max(0, pushed - (halo + delay)), (sizes[:5], pushed, emitted)
            assert lag[-1] == (T, T)
    # the Python binding: same pieces, and the delay beside the halo
    pieces = list(eng.vocoder_stream(cut(mel, [1, 7, 40, 3, 45]), B, denoise_strength=0.0))
    np.testing.assert_array_equal(np.concatenate(pieces, axis=1), want)
    assert eng.stream_delay == C_ and eng.stream_halo == halo
    pcm2 = np.concatenate(list(eng.vocoder_stream(cut(mel, [50, 46]), B, want_pcm=True, denoise_strength=0.0)), axis=1)
    np.testing.assert_array_equal(pcm2, want_pcm)
    eng.set_precision("fp32")


# 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_raw_abi_two_in_flight_with_one_shot_calls_between(eng, mel):
    load_geometry(eng, 1024, 4)
    rng = np.random.Generator(np.random.PCG64(77))
    _, _, want, want_pcm = one_shot(eng, mel, 0.1)
    other = rng.standard_normal((2, 20, 80)).astype(np.float32)
    o_wav, o_pcm, o_dn, o_dn_pcm = one_shot(eng, other, 0.3)
    o_wav2, o_pcm2 = eng.vocoder(other, 2, 20, channels_first=False, pcm=True)   # the resident one-shot result from here on
    np.testing.assert_array_equal(o_wav2, o_wav)

    def between():   # one-shot calls on other data between the steps: their own results stay what they were ...
        w, p = eng.vocoder(other, 2, 20, channels_first=False, pcm=True)
        np.testing.assert_array_equal(w, o_wav)
        np.testing.assert_array_equal(p, o_pcm)
        dw, dp = eng.denoise(o_wav, None, 0.3, want_pcm=True)
        np.testing.assert_array_equal(dw, o_dn)
        np.testing.assert_array_equal(dp, o_dn_pcm)

    sizes = [16] * 6
    wav, pcm, _, _, _ = stream(eng, mel, sizes, 0.1, between=between)   # ... and the stream's too
    np.testing.assert_array_equal(wav, want)
    np.testing.assert_array_equal(pcm, want_pcm)
    # the resident one-shot wav and PCM are untouched by the stream
    np.testing.assert_array_equal(eng.fetch_wav(2, 20), o_wav)
    res = np.empty_like(o_pcm)
    assert eng.lib.e2etts_fetch_pcm(eng._h, _addr(res), res.size) == E_OK
    np.testing.assert_array_equal(res, o_pcm)

    # call order push, push, fetch, push, fetch ...: a third unfetched push is refused, and the stream goes on
    chunks = cut(mel, sizes)
    halo, delay = begin(eng, B, 0.1)
    assert halo >= 0 and delay == 3
    got, waiting = [], []
    for i, c in enumerate(chunks):
        rc, n = push(eng, c, i == len(chunks) - 1)
        assert rc == E_OK
        if n > 0:
            waiting.append(n)
        if len(waiting) == 2:
            if i + 1 < len(chunks):
                rc3, _ = push(eng, chunks[i + 1], False)
                assert rc3 == E_STATE and "await" in eng.lib.e2etts_last_error(eng._h).decode()
            got.append(fetch(eng, B, waiting.pop(0)))
    while waiting:
        got.append(fetch(eng, B, waiting.pop(0)))
    np.testing.assert_array_equal(np.concatenate([g[0] for g in got], axis=1), want)
    np.testing.assert_array_equal(np.concatenate([g[1] for g in got], axis=1), want_pcm)
    assert eng.lib.e2etts_vocoder_stream_fetch(eng._h, _addr(np.empty((B, 1 << 16), np.float32)), None, B << 16) == E_STATE   # nothing left


# 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_short_streams(eng, mel):
    load_geometry(eng, 1024, 4)
    for t in (1, 2):   # 256 and 512 samples <= filter_length / 2: copied through, as e2etts_denoise does with a row it cannot reflect
        m = np.ascontiguousarray(mel[:, :t])
        voc, voc_pcm, want, want_pcm = one_shot(eng, m, 0.1)
        np.testing.assert_array_equal(want, voc)
        for sizes in ([t], [1] * t):
            wav, pcm, _, _, _ = stream(eng, m, sizes, 0.1)
            np.testing.assert_array_equal(wav, voc)
            np.testing.assert_array_equal(pcm, np.trunc(voc * np.float32(32768.0)).clip(-32768, 32767).astype(np.int16))
            np.testing.assert_array_equal(pcm, want_pcm)
    m = np.ascontiguousarray(mel[:, :3])   # 768 samples: the first length that is denoised
    voc, _, want, want_pcm = one_shot(eng, m, 0.1)
    assert (want != voc).any()
    for sizes in ([3], [1, 1, 1], [2, 1]):
        wav, pcm, _, _, _ = stream(eng, m, sizes, 0.1)
        np.testing.assert_array_equal(wav, want)
        np.testing.assert_array_equal(pcm, want_pcm)


# 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_stream_against_the_references_own_output():
    """Fixture c: the tiny vocoder with the fixture's weights, the reference's bias spectrum, the fixture's mel (T = 10), streamed; against
    the reference's float64 run at the bars of test_gpu_denoiser.py::test_vocoder_audio_with_the_references_bias (mean-L1 <= 4 x c_dref,
    max-abs <= 8 x c_dmax, int16 within 1 LSB on >= 99.9 % of the samples)."""
    gold = load_golden("denoiser")
    e = new_engine(seed=int(gold["c_weight_seed"]))
    load_geometry(e, 1024, 4, bias=gold["c_bias_spec"])
    m = np.ascontiguousarray(gold["c_mel"].transpose(0, 2, 1))
    assert m.shape == (2, 10, 80)
    s, dref, dmax = float(gold["c_strength"]), float(gold["c_dref"]), float(gold["c_dmax"])
    want32 = np.trunc(gold["c_out32"].astype(np.float32) * np.float32(32768.0)).clip(-32768, 32767).astype(np.int32)
    for sizes in ([3, 3, 4], [10]):
        wav, pcm, _, _, _ = stream(e, m, sizes, s)
        d = np.abs(wav.astype(np.float64) - gold["c_out64"])
        frac = float((np.abs(pcm.astype(np.int32) - want32) <= 1).mean())
        print(f"stream {sizes} vs reference float64: mean-L1 {d.mean():.3e} (bar {4 * dref:.3e}) max {d.max():.3e} (bar {8 * dmax:.3e}); "
              f"int16 within 1 LSB {100 * frac:.3f} %")
        assert d.mean() <= 4 * dref and d.max() <= 8 * dmax
        assert frac >= 0.999
    e.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_48k_geometry_plain_bf16():
    from test_gpu_longform import cfg48, make_engine
    _, e = make_engine(cfg48(64), 32)
    e.set_precision("bf16")
    load_geometry(e, 1024, 4)
    m = np.random.Generator(np.random.PCG64(48)).standard_normal((2, 70, 80)).astype(np.float32)
    _, _, want, want_pcm = one_shot(e, m, 0.1)
    wav, pcm, _, delay, _ = stream(e, m, [16] * 4 + [6], 0.1)
    assert delay == 2 == dn.stream_delay_frames(1024, 256, 512)
    np.testing.assert_array_equal(wav, want)
    np.testing.assert_array_equal(pcm, want_pcm)


# 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(mel):
    e = new_engine()
    lib, h = e.lib, e._h
    fwd, inv, _ = dn.stft_bases(1024, 256, 1024)
    bias = np.full(513, 0.25, np.float32)
    assert begin(e, B, 0.1)[0] == E_STATE and b"bases" in lib.e2etts_last_error(h)
    assert lib.e2etts_denoiser_load(h, _addr(fwd), _addr(inv), None, 1024, 256) == E_OK
    assert begin(e, B, 0.1)[0] == E_STATE and b"bias" in lib.e2etts_last_error(h)
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), 513) == E_OK
    assert begin(e, B, -0.5)[0] == E_INVAL
    assert begin(e, B, float("nan"))[0] == E_INVAL
    # a denoiser hop that does not divide hop_length (256): 512 x 2
    f2, i2, _ = dn.stft_bases(1024, 512, 1024)
    assert lib.e2etts_denoiser_load(h, _addr(f2), _addr(i2), None, 1024, 512) == E_OK
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), 513) == E_OK
    assert begin(e, B, 0.1)[0] == E_INVAL and b"hop_length" in lib.e2etts_last_error(h)
    assert lib.e2etts_denoiser_load(h, _addr(fwd), _addr(inv), None, 1024, 256) == E_OK
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), 513) == E_OK
    # nothing was opened by a refused call
    assert push(e, np.ascontiguousarray(mel[:, :8]), False)[0] == E_STATE
    _, _, want, want_pcm = one_shot(e, mel, 0.1)

    # while a denoised stream is open its chunks read the bases and the bias: they cannot be replaced
    chunks = cut(mel, [40, 30, 26])
    assert begin(e, B, 0.1)[0] >= 0
    rc, n0 = push(e, chunks[0], False)
    assert rc == E_OK and n0 > 0
    assert lib.e2etts_denoiser_load(h, _addr(f2), _addr(i2), None, 1024, 512) == E_STATE
    assert lib.e2etts_denoiser_set_bias(h, _addr(np.ones(513, np.float32)), 513) == E_STATE
    assert lib.e2etts_denoiser_calibrate(h, None, 88, None) == E_STATE
    got = [fetch(e, B, n0)]
    rc, n1 = push(e, chunks[1], False)
    assert rc == E_OK and n1 > 0
    rc, n2 = push(e, chunks[2], True)
    assert rc == E_OK and n2 > 0
    assert lib.e2etts_denoiser_set_bias(h, _addr(np.ones(513, np.float32)), 513) == E_STATE   # the last chunks are still in flight
    got += [fetch(e, B, n1), fetch(e, B, n2)]
    np.testing.assert_array_equal(np.concatenate([g[0] for g in got], axis=1), want)
    np.testing.assert_array_equal(np.concatenate([g[1] for g in got], axis=1), want_pcm)
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), 513) == E_OK   # finished: free again

    # a weight reload closes a denoised stream like any other
    assert begin(e, B, 0.1)[0] >= 0
    assert push(e, chunks[0], False)[0] == E_OK
    from e2e_tts_amd import packer
    e.load_weights(packer.pack(e.dims, _STATE["ac"], sw.make_vocoder_state(cfgmod.tiny_config(), seed=99)))
    rc, _ = push(e, chunks[1], False)
    assert rc == E_STATE and b"no open vocoder stream" in lib.e2etts_last_error(h)
    assert lib.e2etts_denoiser_set_bias(h, _addr(bias), 513) == E_OK   # ... and the denoiser is free
    wav, pcm, _, _, _ = stream(e, mel, [50, 46], 0.1)
    _, _, want2, _ = one_shot(e, mel, 0.1)
    np.testing.assert_array_equal(wav, want2)
    assert (want2 != want).any()
    e.close()


def test_istft_tail_is_refused():
    from e2e_tts_amd.models import iSTFT
    cfg = cfgmod.tiny_config()
    v = iSTFT(cfg["models"]["istft"])
    v.load_state_dict(sw.to_torch(sw.make_vocoder_state(cfg, seed=5, vocoder="istft")))
    e = v.eval().to(0).engine
    assert e.dims.hop_length % 256 == 0
    load_geometry(e, 1024, 4)
    rc, _ = begin(e, 1, 0.1)
    assert rc == E_INVAL and b"iSTFT" in e.lib.e2etts_last_error(e._h)
    assert e.lib.e2etts_vocoder_stream_begin(e._h, 1) >= 0   # the plain stream serves it as before


# 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_plain_begin_is_never_denoised(eng, mel):
    load_geometry(eng, 1024, 4)
    voc, voc_pcm = eng.vocoder(mel, B, T, channels_first=False, pcm=True)
    # a denoised stream first, so that the engine's stream state has been a denoised one
    begin(eng, B, 0.1)
    try:
        eng.set_denoise(0.1)
        wav = np.concatenate(list(eng.vocoder_stream(cut(mel, [1, 7, 40, 3, 45]), B)), axis=1)
        pcm = np.concatenate(list(eng.vocoder_stream(cut(mel, [50, 46]), B, want_pcm=True)), axis=1)
    finally:
        eng.set_denoise(0.0)
    np.testing.assert_array_equal(wav, voc)
    np.testing.assert_array_equal(pcm, voc_pcm)
    assert eng.stream_delay == 0
    # ... and a denoised stream is denoised without e2etts_set_denoise
    _, _, want, _ = one_shot(eng, mel, 0.1)
    got, _, _, _, _ = stream(eng, mel, [50, 46], 0.1)
    np.testing.assert_array_equal(got, want)
    assert (want != voc).any()


# 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_models_denoiser_stream():
    import torch
    from e2e_tts_amd.models import Denoiser, HifiGan
    cfg = cfgmod.tiny_config()
    v = HifiGan(cfg["models"]["hifigan"], device=0)
    v.load_state_dict(sw.to_torch(sw.make_vocoder_state(cfg, seed=4321)))
    v.eval()
    den = Denoiser(v)
    m = np.random.Generator(np.random.PCG64(8)).standard_normal((2, 40, 80)).astype(np.float32)
    want = den(v(torch.from_numpy(np.ascontiguousarray(m.transpose(0, 2, 1)))).squeeze(1), strength=0.2)[:, 0].cpu().numpy()
    got = np.concatenate(list(den.stream(cut(m, [13, 1, 26]), strength=0.2)), axis=1)
    np.testing.assert_array_equal(got, want)
    pcm = np.concatenate(list(den.stream(iter(cut(m, [20, 20])), strength=0.2, want_pcm=True)), axis=1)
    assert pcm.dtype == np.int16
    _, want_pcm = v.engine.denoise(v.engine.vocoder(m, 2, 40, channels_first=False)[0], None, 0.2, want_pcm=True)
    np.testing.assert_array_equal(pcm, want_pcm)
    assert list(den.stream([])) == []
    with pytest.raises(ValueError):
        list(den.stream([m[:, :, :40]]))
