"""GPU tests (-m gpu) of the vocoder precision "fp16_act" (E2ETTS_PRECISION_FP16_ACT, include/e2etts.h): every vocoder activation in
fp16, rounded where the reference's HifiGan run with .half() rounds.  They mirror tests/test_gpu_bf16_act.py case for case.

The engine is pinned to the CPU restatement of the header's rounding table with the engine's own parameters (tests/act16_ref.py,
dtype=torch.float16, weights="engine").  What may differ is the order of fp32 accumulation inside each convolution: a one-ulp flip of a
layer output, which the later layers spread.  How large that gets is measured on the CPU, per case, as the distance between the
restatement with fp32 and with fp64 accumulation; the engine must stay within twice that.  On the deep generators the floor is 0.78 x ..
0.88 x of the reference's own fp16-vs-fp32 distance (tests/test_fp16_act_host.py); on the shallow one it is 0.108 x, so that bar
(0.22 x) lies below the 0.30 x where a dropped rounding point lands: the shallow case is the sharp one."""
import numpy as np
import pytest
import torch

from conftest import load_golden, states_for
from e2e_tts_amd import config as cfgmod, synth_weights as sw

pytestmark = pytest.mark.gpu

CASES = ("48k_w512", "22k_v1", "22k_rb2", "shallow")


def cfg48(width):
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=width)
    cfg["audio"]["stft"]["hop_length"] = 512
    cfg["audio"]["signal"]["sampling_rate"] = 48000
    return cfg


def make(cfg, seed):
    from e2e_tts_amd.models import HifiGan
    state = sw.make_vocoder_state(cfg, seed=seed)
    v = HifiGan(cfg["models"]["hifigan"])
    v.load_state_dict(sw.to_torch(state))
    return state, v


def mean_l1(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean())


def is_fp16(x):
    x = np.asarray(x, np.float32)
    return np.array_equal(x.astype(np.float16).astype(np.float32), x)


@pytest.mark.parametrize("case", CASES)
def test_engine_matches_restatement(case):
    """Every fixture case, the shallow generator (width 64, one upsampler of rate 2, one ResBlock1 of kernel 3) included: the engine
    serves that geometry as the issue states it."""
    from act16_ref import Act16Vocoder, fixture_case
    g = load_golden("hifigan_fp16")
    cfg, state, mel = fixture_case(g, case)
    _, v = make(cfg, int(g[f"{case}.weight_seed"]))
    eng = v.to(0).engine
    eng.set_precision("fp16_act")
    B, T = mel.shape[:2]
    wav, pcm = eng.vocoder(mel, B, T, channels_first=False, pcm=True)
    assert np.isfinite(wav).all() and is_fp16(wav)
    np.testing.assert_array_equal(pcm, (wav * np.float32(32768.0)).astype(np.int32).astype(np.int16))
    hg = cfg["models"]["hifigan"]
    ref = Act16Vocoder(state, hg, weights="engine").forward(mel)
    ref64 = Act16Vocoder(state, hg, weights="engine", acc=torch.float64).forward(mel)
    unit = float(g[f"{case}.ref_fp16_mean_l1"])
    d, floor = mean_l1(wav, ref), mean_l1(ref, ref64)
    msg = f"{case}: engine vs restatement {d:.3e} ({d / unit:.3f} x), accumulation-order floor {floor:.3e} ({floor / unit:.3f} x)"
    if int(hg.get("resblock", 1)) == 1:
        from oracle.ref_numpy import VocoderOracle
        f32 = VocoderOracle(state, cfg).forward(np.ascontiguousarray(mel.transpose(0, 2, 1)))[:, 0]
        msg += f", restatement vs fp32 oracle {mean_l1(ref, f32):.3e}, engine vs fp32 oracle {mean_l1(wav, f32):.3e}"
        print(msg)
        assert mean_l1(wav, f32) < 1.5 * mean_l1(ref, f32), msg
    print(msg)
    assert d <= 2.0 * floor + 1e-7, msg
    eng.close()


def test_dropin_half_on_reference_fixture():
    """HifiGan(cfg).load_state_dict(sd).half() on mel.half(): the reference's own call, with a torch.float16 tensor out."""
    from act16_ref import Act16Vocoder, fixture_case
    g = load_golden("hifigan_fp16")
    tag = "48k_w512"
    cfg, _, mel_btc = fixture_case(g, tag)
    state, v = make(cfg, int(g[f"{tag}.weight_seed"]))
    mel = torch.from_numpy(np.ascontiguousarray(mel_btc.transpose(0, 2, 1)))
    assert v.half() is v                      # before the engine exists: selected when it is created
    out = v(mel.half())
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 90 * 512) and out.is_cuda
    wav = out.float().cpu().numpy()[:, 0]
    assert is_fp16(wav)
    out32 = v(mel)                            # an fp32 mel is staged as fp16(mel): the same bits
    assert out32.dtype == torch.float16 and torch.equal(out32, out)
    ref16, ref32, unit = g[f"{tag}.wav_ref_fp16"].astype(np.float32), g[f"{tag}.wav"], float(g[f"{tag}.ref_fp16_mean_l1"])
    assert v.bfloat16() is v
    wav_b = v(mel.bfloat16())
    assert wav_b.dtype == torch.bfloat16
    wav_b = wav_b.float().cpu().numpy()[:, 0]
    assert v.float() is v
    assert v(mel).dtype == torch.float32      # .float() leaves the mode
    v.half()
    np.testing.assert_array_equal(v(mel.half()).float().cpu().numpy()[:, 0], wav)
    # the bar: the restatement's distance with the module's weights plus the weight-path margin recorded by the host test
    # (test_fp16_act_host.MEASURED[tag]["engine"]: with the engine's weights the restatement lies 1.200 x from wav_ref_fp16).  Printed
    # beside it: the restatement with the ENGINE's weights, which the engine matches up to accumulation order (measured on the MI355X:
    # engine 1.206 x, restatement with engine weights 1.207 x -- a tie that accumulation-order flips decide either way).
    from test_fp16_act_host import MEASURED
    hg = cfg["models"]["hifigan"]
    d_mod = mean_l1(Act16Vocoder(state, hg, weights="module").forward(mel_btc), ref16)
    d_eng = mean_l1(Act16Vocoder(state, hg, weights="engine").forward(mel_btc), ref16)
    margin = MEASURED[tag]["engine"] * unit
    d4, df, dfb = mean_l1(wav, ref16), mean_l1(wav, ref32), mean_l1(wav_b, ref32)
    print(f"{tag} vs wav_ref_fp16: fp16_act {d4 / unit:.3f} x, restatement with module weights {d_mod / unit:.3f} x, with engine weights "
          f"{d_eng / unit:.3f} x (recorded weight-path margin {margin / unit:.3f} x); vs fp32 wav: fp16_act {df / unit:.3f} x = {df:.3e}, "
          f"bf16_act {dfb / unit:.3f} x = {dfb:.3e}")
    assert d4 <= d_mod + margin
    assert df <= 1.5 * unit
    assert df < dfb
    v.engine.close()


def test_bit_for_bit_invariants():
    g = load_golden("hifigan_48k")
    cfg = cfg48(512)
    _, v = make(cfg, int(g["w512.weight_seed"]))
    eng = v.to(0).engine
    rng = np.random.Generator(np.random.PCG64(22))
    T = 333
    mel = rng.standard_normal((3, T, 80)).astype(np.float32)
    before = {}
    for prec in ("bf16", "bf16_act"):
        eng.set_precision(prec)
        before[prec], _ = eng.vocoder(mel[:1], 1, T, channels_first=False)
    eng.set_precision("fp16_act")
    whole, whole_pcm = eng.vocoder(mel, 3, T, channels_first=False, pcm=True)
    assert np.isfinite(whole).all() and is_fp16(whole)
    # fusion levels 0 / 1 / 2
    for lvl in (0, 1):
        eng.set_fused_resblocks(lvl)
        again, _ = eng.vocoder(mel, 3, T, channels_first=False)
        np.testing.assert_array_equal(again, whole, err_msg=f"fusion level {lvl}")
    eng.set_fused_resblocks(2)
    # one row of the batch = that utterance alone
    one, _ = eng.vocoder(np.ascontiguousarray(mel[1:2]), 1, T, channels_first=False)
    np.testing.assert_array_equal(one[0], whole[1])
    # stream == one-shot (push(i + 1) before fetch(i): Engine.vocoder_stream keeps two chunks in flight)
    for sizes in ([T], [1, 7, 40, 3, 100, 2, 180], [16] * 20 + [13], [200, 133]):
        chunks, pos = [], 0
        for n in sizes:
            chunks.append(np.ascontiguousarray(mel[:, pos:pos + n]))
            pos += n
        out = np.concatenate(list(eng.vocoder_stream(chunks, 3)), axis=1)
        np.testing.assert_array_equal(out, whole, err_msg=str(sizes))
    pcm = np.concatenate(list(eng.vocoder_stream([np.ascontiguousarray(mel[:, :150]), np.ascontiguousarray(mel[:, 150:])], 3, want_pcm=True)), axis=1)
    np.testing.assert_array_equal(pcm, whole_pcm)
    # bf16_act -> fp16_act -> bf16_act and bf16 -> fp16_act -> bf16: the bits of before, and of a fresh engine
    for prec in ("bf16_act", "bf16"):
        eng.set_precision(prec)
        after, _ = eng.vocoder(mel[:1], 1, T, channels_first=False)
        np.testing.assert_array_equal(after, before[prec], err_msg=prec)
        eng.set_precision("fp16_act")
        again, _ = eng.vocoder(mel[:1], 1, T, channels_first=False)
        np.testing.assert_array_equal(again[0], whole[0], err_msg=f"fp16_act after {prec}")
    _, v2 = make(cfg, int(g["w512.weight_seed"]))
    e2 = v2.to(0).engine
    for prec in ("bf16_act", "bf16"):
        e2.set_precision(prec)
        fresh, _ = e2.vocoder(mel[:1], 1, T, channels_first=False)
        np.testing.assert_array_equal(fresh, before[prec], err_msg=f"fresh engine, {prec}")
    e2.close()
    eng.close()


def test_ragged_on_equals_off_on_valid_samples():
    from e2e_tts_amd.runtime import engine_from_states
    g = load_golden("full_b3")
    cfg, ac, voc = states_for(g, "full_b3")
    eng = engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, voc, device=0)
    eng.set_precision("fp16_act")
    spk = np.array([int(g["speaker"])], np.int64)
    hop = cfg["audio"]["stft"]["hop_length"]
    outs = {}
    for ragged in (False, True):
        eng.set_ragged(ragged)
        outs[ragged] = eng.synthesize(g["ids"], g["lens"], spk)
    (a, ml, T), (b, ml2, T2) = outs[False], outs[True]
    assert T == T2 and (ml == ml2).all() and len(set(int(x) for x in ml)) > 1, ml
    for r, n in enumerate(ml * hop):
        np.testing.assert_array_equal(b[r, :n], a[r, :n])
    eng.close()


def test_workspace_halves():
    """Growth of device_bytes between two windows (48 kHz, width 512, B = 1), fresh engines: the weight images drop out of the difference.
    The windows are 4096 and 8192 frames, as in test_gpu_bf16_act.py: both above the size where mode 2 runs the ResBlocks of a stage side
    by side.  fp16_act grows by at most 0.6 x of what bf16 grows by, and by exactly what bf16_act grows by (same bytes per element)."""
    cfg = cfg48(512)
    rng = np.random.Generator(np.random.PCG64(23))
    growth = {}
    for prec in ("bf16", "bf16_act", "fp16_act"):
        sizes = []
        for T in (4096, 8192):
            _, v = make(cfg, 7)
            eng = v.to(0).engine
            eng.set_precision(prec)
            mel = rng.standard_normal((1, T, 80)).astype(np.float32)
            eng.vocoder(mel, 1, T, channels_first=False)
            eng.sync()
            sizes.append(eng.device_bytes())
            eng.close()
        growth[prec] = sizes[1] - sizes[0]
    print("device_bytes growth 4096 -> 8192 frames:", growth)
    assert 0 < growth["fp16_act"] <= 0.6 * growth["bf16"], growth
    assert growth["fp16_act"] == growth["bf16_act"], growth


def test_images_are_built_at_the_first_selection_only():
    """An engine that never selects fp16_act owns nothing of it; selecting it adds the fp16 images and parameters once."""
    _, v = make(cfg48(512), 7)
    eng = v.to(0).engine
    loaded = eng.device_bytes()
    eng.set_precision("bf16_act")
    assert eng.device_bytes() == loaded
    eng.set_precision("fp16_act")
    first = eng.device_bytes()
    assert first > loaded
    eng.set_precision("bf16")
    eng.set_precision("fp16_act")
    assert eng.device_bytes() == first
    print(f"device_bytes after load {loaded}, after the first selection of fp16_act {first} (+{first - loaded})")
    eng.close()


def test_rejections_leave_the_engine_usable():
    from e2e_tts_amd.models import iSTFT
    g = load_golden("hifigan_48k")
    # the w64 generator: 32 / 16 / 8 / 4 channels have no fp16-I/O route
    _, v = make(cfg48(64), int(g["w64.weight_seed"]))
    eng = v.to(0).engine
    eng.set_precision("bf16")
    before, _ = eng.vocoder(g["w64.mel"], 2, 90, channels_first=False)
    with pytest.raises(ValueError, match="fp16_act"):
        eng.set_precision("fp16_act")
    with pytest.raises(ValueError, match="fp16_act"):
        v.half()
    after, _ = eng.vocoder(g["w64.mel"], 2, 90, channels_first=False)
    np.testing.assert_array_equal(after, before)
    # the mode as the decoder precision
    _, v5 = make(cfg48(512), 5)
    e5 = v5.to(0).engine
    e5.set_precision("bf16_act")
    w_before, _ = e5.vocoder(g["w512.mel"], 1, 90, channels_first=False)
    with pytest.raises(ValueError, match="fp16_act"):
        e5.set_precision("bf16", "fp16_act")
    w_after, _ = e5.vocoder(g["w512.mel"], 1, 90, channels_first=False)
    np.testing.assert_array_equal(w_after, w_before)
    e5.set_precision("fp16_act")
    w, _ = e5.vocoder(g["w512.mel"], 1, 90, channels_first=False)
    assert np.isfinite(w).all() and is_fp16(w)
    # the iSTFT tail
    cfg = cfgmod.default_config()
    hg = cfg["models"]["istft"]
    iv = iSTFT(hg)
    with pytest.raises(NotImplementedError):
        iv.half()
    ie = iv.to(0).engine
    with pytest.raises(ValueError, match="fp16_act"):
        ie.set_precision("fp16_act")
    ie.set_precision("fp32")
    for e in (eng, e5, ie):
        e.close()
