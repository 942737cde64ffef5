"""GPU tests (-m gpu) of the vocoder precision "bf16_act" (E2ETTS_PRECISION_BF16_ACT, include/e2etts.h): every vocoder activation in
bf16, rounded where the reference's HifiGan run with .bfloat16() rounds.

The engine is pinned to the CPU restatement of the header's rounding table with the engine's own parameters (tests/bf16_act_ref.py,
weights="engine").  What may differ is the order of fp32 accumulation inside each convolution: a one-ulp flip of a layer output, which
the later layers spread.  How large that gets is measured on the CPU, per case, as the distance between the restatement with fp32 and
with fp64 accumulation; the engine must stay within twice that.  (tests/test_bf16_act_host.py: the floor is 0.37 x / 0.75 x of the
reference's own bf16-vs-fp32 distance at widths 64 / 512.)"""
import numpy as np
import pytest
import torch

from conftest import load_golden, states_for
from e2e_tts_amd import config as cfgmod, synth_weights as sw

pytestmark = pytest.mark.gpu


def cfg48(width):
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=width)
    cfg["audio"]["stft"]["hop_length"] = 512
    cfg["audio"]["signal"]["sampling_rate"] = 48000
    return cfg


def cfg_rb2():
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(resblock=2, resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])
    return cfg


def make(cfg, seed):
    from e2e_tts_amd.models import HifiGan
    state = sw.make_vocoder_state(cfg, seed=seed)
    v = HifiGan(cfg["models"]["hifigan"])
    v.load_state_dict(sw.to_torch(state))
    return state, v


def mean_l1(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean())


def is_bf16(x):
    x = np.asarray(x, np.float32)
    return np.array_equal(torch.from_numpy(x).bfloat16().float().numpy(), x)


def _cases():
    g = load_golden("hifigan_48k")
    rng = np.random.Generator(np.random.PCG64(21))
    return {
        "48k_w512": (cfg48(512), int(g["w512.weight_seed"]), g["w512.mel"]),
        "22k_v1": (cfgmod.default_config(), 41, rng.standard_normal((2, 40, 80)).astype(np.float32)),
        "22k_resblock2": (cfg_rb2(), 42, rng.standard_normal((1, 48, 80)).astype(np.float32)),
    }


@pytest.mark.parametrize("case", ["48k_w512", "22k_v1", "22k_resblock2"])
def test_engine_matches_restatement(case):
    from bf16_act_ref import Bf16ActVocoder
    cfg, seed, mel = _cases()[case]
    state, v = make(cfg, seed)
    eng = v.to(0).engine
    eng.set_precision("bf16_act")
    B, T = mel.shape[:2]
    wav, pcm = eng.vocoder(mel, B, T, channels_first=False, pcm=True)
    assert is_bf16(wav)
    np.testing.assert_array_equal(pcm, (wav * np.float32(32768.0)).astype(np.int32).astype(np.int16))
    hg = cfg["models"]["hifigan"]
    ref = Bf16ActVocoder(state, hg, weights="engine").forward(mel)
    ref64 = Bf16ActVocoder(state, hg, weights="engine", acc=torch.float64).forward(mel)
    d, floor = mean_l1(wav, ref), mean_l1(ref, ref64)
    msg = f"{case}: engine vs restatement {d:.3e}, accumulation-order floor {floor:.3e}"
    if int(hg.get("resblock", 1)) == 1:
        from oracle.ref_numpy import VocoderOracle
        f32 = VocoderOracle(state, cfg).forward(np.ascontiguousarray(mel.transpose(0, 2, 1)))[:, 0]
        msg += f", restatement vs fp32 oracle {mean_l1(ref, f32):.3e}, engine vs fp32 oracle {mean_l1(wav, f32):.3e}"
        assert mean_l1(wav, f32) < 1.5 * mean_l1(ref, f32), msg
    print(msg)
    assert d <= 2.0 * floor + 1e-7, msg


def test_dropin_bfloat16_on_reference_fixture():
    """HifiGan(cfg).load_state_dict(sd).bfloat16() on mel.bfloat16(): the reference's own call, with a bf16 tensor out."""
    from bf16_act_ref import Bf16ActVocoder
    g = load_golden("hifigan_48k")
    cfg = cfg48(512)
    state, v = make(cfg, int(g["w512.weight_seed"]))
    mel = torch.from_numpy(np.ascontiguousarray(g["w512.mel"].transpose(0, 2, 1)))
    assert v.bfloat16() is v
    out = v(mel.bfloat16())
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, 1, 90 * 512) and out.is_cuda
    wav = out.float().cpu().numpy()[:, 0]
    ref16, ref32, unit = g["w512.wav_ref_bf16"], g["w512.wav"], float(g["w512.ref_bf16_mean_l1"])
    v.float()
    eng = v.engine
    eng.set_precision("bf16")
    wav2, _ = eng.vocoder(g["w512.mel"], 1, 90, channels_first=False)
    v.bfloat16()
    # the margin: what the weight path alone costs (restatement with the engine's parameters against the module's, host test 3)
    margin = (mean_l1(Bf16ActVocoder(state, cfg["models"]["hifigan"], weights="engine").forward(g["w512.mel"]), ref16) -
              mean_l1(Bf16ActVocoder(state, cfg["models"]["hifigan"], weights="module").forward(g["w512.mel"]), ref16))
    d3, d2, df = mean_l1(wav, ref16), mean_l1(wav2, ref16), mean_l1(wav, ref32)
    print(f"w512 vs wav_ref_bf16: bf16_act {d3 / unit:.3f} x, bf16 {d2 / unit:.3f} x (weight-path margin {margin / unit:.3f} x); "
          f"bf16_act vs fp32 wav {df / unit:.3f} x ref_bf16_mean_l1")
    assert d3 < d2 + max(margin, 0.0)
    assert df <= 1.5 * unit


def test_bit_for_bit_invariants():
    g = load_golden("hifigan_48k")
    cfg = cfg48(512)
    _, v = make(cfg, int(g["w512.weight_seed"]))
    eng = v.to(0).engine
    rng = np.random.Generator(np.random.PCG64(22))
    T = 333
    mel = rng.standard_normal((3, T, 80)).astype(np.float32)
    eng.set_precision("bf16")
    m2_before, _ = eng.vocoder(mel[:1], 1, T, channels_first=False)
    eng.set_precision("bf16_act")
    whole, whole_pcm = eng.vocoder(mel, 3, T, channels_first=False, pcm=True)
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
    # 2 -> 3 -> 2: the mode-2 bits of before, and of a fresh engine
    eng.set_precision("bf16")
    m2_after, _ = eng.vocoder(mel[:1], 1, T, channels_first=False)
    np.testing.assert_array_equal(m2_after, m2_before)
    _, v2 = make(cfg, int(g["w512.weight_seed"]))
    e2 = v2.to(0).engine
    e2.set_precision("bf16")
    m2_fresh, _ = e2.vocoder(mel[:1], 1, T, channels_first=False)
    np.testing.assert_array_equal(m2_fresh, m2_before)
    e2.close()


def test_ragged_on_equals_off_on_valid_samples():
    from e2e_tts_amd.runtime import engine_from_states
    g = load_golden("full_b3")
    cfg, ac, voc = states_for(g, "full_b3")
    eng = engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, voc, device=0)
    eng.set_precision("bf16_act")
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
    The windows are 4096 and 8192 frames, both above the size where mode 2 runs the ResBlocks of a stage side by side (2048 frames): below
    it, mode 2 also holds six side-stream buffers that mode 3 does not have, and a difference across that boundary (512 -> 4096: 0.64 x,
    computed from the buffer sizes) measures those rather than the element size."""
    cfg = cfg48(512)
    rng = np.random.Generator(np.random.PCG64(23))
    growth = {}
    for prec in ("bf16", "bf16_act"):
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
    assert 0 < growth["bf16_act"] <= 0.6 * growth["bf16"], growth


def test_rejections_leave_the_engine_usable():
    from e2e_tts_amd.models import iSTFT
    g = load_golden("hifigan_48k")
    # the w64 generator: 32 / 16 / 8 / 4 channels have no bf16-I/O route
    _, v = make(cfg48(64), int(g["w64.weight_seed"]))
    eng = v.to(0).engine
    eng.set_precision("bf16")
    before, _ = eng.vocoder(g["w64.mel"], 2, 90, channels_first=False)
    with pytest.raises(ValueError):
        eng.set_precision("bf16_act")
    with pytest.raises(ValueError):
        v.bfloat16()
    after, _ = eng.vocoder(g["w64.mel"], 2, 90, channels_first=False)
    np.testing.assert_array_equal(after, before)
    # mode 3 as the decoder precision
    _, v5 = make(cfg48(512), 5)
    e5 = v5.to(0).engine
    with pytest.raises(ValueError):
        e5.set_precision("bf16", "bf16_act")
    e5.set_precision("bf16_act")
    w, _ = e5.vocoder(g["w512.mel"], 1, 90, channels_first=False)
    assert np.isfinite(w).all() and is_bf16(w)
    # the iSTFT tail
    cfg = cfgmod.default_config()
    hg = cfg["models"]["istft"]
    iv = iSTFT(hg)
    with pytest.raises(NotImplementedError):
        iv.bfloat16()
    ie = iv.to(0).engine
    with pytest.raises(ValueError):
        ie.set_precision("bf16_act")
    ie.set_precision("fp32")
    for e in (eng, e5, ie):
        e.close()