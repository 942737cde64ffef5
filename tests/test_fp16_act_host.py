"""Vocoder precision "fp16_act" (E2ETTS_PRECISION_FP16_ACT) on the host: the C ABI constant and the Python table agree, and the CPU
restatement of its rounding table (tests/act16_ref.py with dtype=torch.float16) reproduces the reference's own HifiGan run with .half()
(fixture hifigan_fp16: wav_ref_fp16, tools/make_fp16_goldens.py) as closely as accumulation order allows.

Distances are wav mean-L1 in units of the case's ref_fp16_mean_l1 (the reference's .half() run against its fp32 run: 7.6e-5 .. 1.6e-4).
"Floor" is the restatement with fp32 against fp64 accumulation: what one-ulp flips of single layer outputs grow to through the later
layers.  torch's CPU fp16 kernels sum in an order of their own, so no restatement gets closer to wav_ref_fp16 than that.

Measured on the CPU (MEASURED below; every bar is twice the measured value):
  * deep generators (48k_w512, 22k_v1, 22k_rb2): the restatement with module weights lies 0.80 x .. 0.88 x from wav_ref_fp16 and the
    floor is the same size (0.79 x .. 0.88 x): in fp16 the flips grow to the whole distance over four stages.  These cases pin the
    level, not single rounding points: without the round after c1 + b1 they move from 0.877 x to 0.879 x (48k) and 0.803 x to 0.785 x.
  * shallow generator (one upsampler, one ResBlock1): 0.124 x with a floor of 0.122 x (module weights; 0.108 x with the engine's);
    without the round after c1 + b1 it lies 0.312 x away -- outside the bar of 0.248 x.  This is the case that sees a rounding point.
  * engine weights (fp16 of the fp32 weight-norm fold) instead of the module's (weight norm evaluated in fp16): 1.20 x .. 1.32 x from
    wav_ref_fp16 -- the weight path's margin of the GPU drop-in test -- and 0.75 x .. 0.91 x from the reference's fp32 wav."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("48k_w512", "22k_v1", "22k_rb2", "shallow")
# restatement (weights="module") vs wav_ref_fp16; fp32 vs fp64 accumulation (weights="module"); the same without the round after c1 + b1;
# engine weights vs wav_ref_fp16 and vs the reference's fp32 wav -- all in units of ref_fp16_mean_l1
MEASURED = {
    "48k_w512": dict(module=0.877, floor=0.883, drop_c1=0.879, engine=1.200, engine_fp32=0.868),
    "22k_v1": dict(module=0.803, floor=0.792, drop_c1=0.785, engine=1.215, engine_fp32=0.905),
    "22k_rb2": dict(module=0.798, floor=0.787, drop_c1=None, engine=1.316, engine_fp32=0.853),
    "shallow": dict(module=0.124, floor=0.122, drop_c1=0.312, engine=1.215, engine_fp32=0.754),
}


def mean_l1(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean())


def restate(tag, **kw):
    from act16_ref import Act16Vocoder, fixture_case
    g = load_golden("hifigan_fp16")
    cfg, state, mel = fixture_case(g, tag)
    return g, Act16Vocoder(state, cfg["models"]["hifigan"], dtype=torch.float16, **kw).forward(mel)


def test_precision_constant_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "e2etts.h")).read()
    m = re.search(r"#define\s+E2ETTS_PRECISION_FP16_ACT\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 4
    from e2e_tts_amd import _lib
    assert _lib.PRECISIONS == {"fp32": 0, "bf16x3": 1, "bf16": 2, "bf16_act": 3}
    assert _lib.VOCODER_PRECISIONS == {**_lib.PRECISIONS, "fp16_act": 4}
    assert int(re.search(r"#define\s+E2ETTS_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_half_selects_the_mode_before_the_engine_exists():
    from e2e_tts_amd import config as cfgmod
    from e2e_tts_amd.models import HifiGan, iSTFT
    cfg = cfgmod.default_config()
    v = HifiGan(cfg["models"]["hifigan"])
    assert v.half() is v and v._fp16 and not getattr(v, "_bf16", False) and v._engine is None
    assert v.bfloat16() is v and v._bf16 and not v._fp16
    v.half()
    assert v.float() is v and not v._fp16 and not v._bf16
    with pytest.raises(NotImplementedError):
        iSTFT(cfg["models"]["istft"]).half()


def test_fixture_holds_the_issue_cases():
    g = load_golden("hifigan_fp16")
    shapes = {"48k_w512": (1, 90, 512), "22k_v1": (2, 40, 256), "22k_rb2": (1, 48, 256), "shallow": (2, 300, 2)}
    for tag, (B, T, hop) in shapes.items():
        assert g[f"{tag}.mel"].shape == (B, T, 80) and int(g[f"{tag}.hop"]) == hop
        assert g[f"{tag}.wav"].shape == (B, T * hop) and g[f"{tag}.wav"].dtype == np.float32
        assert g[f"{tag}.wav_ref_fp16"].shape == (B, T * hop) and g[f"{tag}.wav_ref_fp16"].dtype == np.float16
        assert np.isfinite(g[f"{tag}.wav_ref_fp16"].astype(np.float32)).all()
        assert float(g[f"{tag}.ref_fp16_mean_l1"]) == pytest.approx(mean_l1(g[f"{tag}.wav_ref_fp16"], g[f"{tag}.wav"]), rel=1e-12)
    assert int(g["48k_w512.upsample_initial_channel"]) == 512 and int(g["22k_rb2.resblock"]) == 2
    assert int(g["shallow.upsample_initial_channel"]) == 64 and g["shallow.upsample_rates"].tolist() == [2]
    assert g["shallow.upsample_kernel_sizes"].tolist() == [4] and g["shallow.resblock_kernel_sizes"].tolist() == [3]
    assert g["shallow.resblock_dilation_sizes"].tolist() == [[1, 3, 5]] and int(g["shallow.resblock"]) == 1
    assert int(g["shallow.weight_seed"]) == 51 and int(g["shallow.mel_seed"]) == 61
    # the parity bar for wav is 1e-4: the reference's .half() run meets it on the served generators
    for tag in ("48k_w512", "22k_v1", "22k_rb2"):
        assert float(g[f"{tag}.ref_fp16_mean_l1"]) <= 1e-4


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_reference_fp16_run(tag):
    g, wav = restate(tag, weights="module")
    ref16, unit = g[f"{tag}.wav_ref_fp16"].astype(np.float32), float(g[f"{tag}.ref_fp16_mean_l1"])
    d = mean_l1(wav, ref16) / unit
    print(f"{tag}: restatement (module weights) vs the reference's .half() run: {d:.3f} x ref_fp16_mean_l1")
    assert d <= 2.0 * MEASURED[tag]["module"], d
    # every value is an fp16 value
    assert np.array_equal(torch.from_numpy(wav).half().float().numpy(), wav)


def test_missing_rounding_point_breaks_the_bar_on_the_shallow_generator():
    """Leaving out the rounding after c1 + b1 moves the shallow generator past its bar; the full table is within it."""
    g, full = restate("shallow", weights="module")
    _, wav = restate("shallow", weights="module", drop=("c1",))
    ref16, unit = g["shallow.wav_ref_fp16"].astype(np.float32), float(g["shallow.ref_fp16_mean_l1"])
    d_full, d = mean_l1(full, ref16) / unit, mean_l1(wav, ref16) / unit
    print(f"shallow: full table {d_full:.3f} x, without the round after c1 + b1 {d:.3f} x")
    assert d_full <= 2.0 * MEASURED["shallow"]["module"] < d, (d_full, d)


@pytest.mark.parametrize("tag", CASES)
def test_record_engine_weight_path_gap(tag):
    """The engine's parameters (fp16 of the fp32 weight-norm fold) against the module's (weight norm in fp16): the extra distance from
    wav_ref_fp16 that the weight path alone causes (printed; the drop-in GPU test allows it as its margin), and the distance to the
    reference's fp32 wav, which must stay within 1.5 x ref_fp16_mean_l1."""
    g, eng_w = restate(tag, weights="engine")
    _, mod_w = restate(tag, weights="module")
    unit, ref16 = float(g[f"{tag}.ref_fp16_mean_l1"]), g[f"{tag}.wav_ref_fp16"].astype(np.float32)
    d_eng, d_mod = mean_l1(eng_w, ref16) / unit, mean_l1(mod_w, ref16) / unit
    d_fp32 = mean_l1(eng_w, g[f"{tag}.wav"]) / unit
    print(f"{tag}: vs wav_ref_fp16, engine weights {d_eng:.3f} x, module weights {d_mod:.3f} x; engine weights vs fp32 wav {d_fp32:.3f} x")
    assert d_fp32 <= 1.5
    assert d_eng <= 2.0 * MEASURED[tag]["engine"]


@pytest.mark.parametrize("tag", CASES)
def test_accumulation_order_floor(tag):
    """fp32 against fp64 accumulation, same rounding table: the size of what one-ulp flips grow to (the floor quoted above)."""
    g, a = restate(tag, weights="module")
    _, b = restate(tag, weights="module", acc=torch.float64)
    d = mean_l1(a, b) / float(g[f"{tag}.ref_fp16_mean_l1"])
    print(f"{tag}: fp32 vs fp64 accumulation: {d:.3f} x ref_fp16_mean_l1")
    assert 0.0 < d < 2.0 * MEASURED[tag]["floor"]


def test_bf16_element_type_is_the_bf16_act_restatement():
    """The parametrised helper with dtype=torch.bfloat16 gives the bits of tests/bf16_act_ref.py (the table is the same with the element
    type exchanged)."""
    from act16_ref import Act16Vocoder, fixture_case
    from bf16_act_ref import Bf16ActVocoder
    g = load_golden("hifigan_fp16")
    for tag in ("shallow", "22k_rb2"):
        cfg, state, mel = fixture_case(g, tag)
        for weights in ("engine", "module"):
            a = Act16Vocoder(state, cfg["models"]["hifigan"], dtype=torch.bfloat16, weights=weights).forward(mel)
            b = Bf16ActVocoder(state, cfg["models"]["hifigan"], weights=weights).forward(mel)
            np.testing.assert_array_equal(a, b)
