"""Vocoder precision "bf16_act" (E2ETTS_PRECISION_BF16_ACT) on the host: the C ABI constant and the Python table agree, and the CPU
restatement of its rounding table (tests/bf16_act_ref.py) reproduces the reference's own HifiGan run with .bfloat16() (fixture
hifigan_48k: wav_ref_bf16) as closely as accumulation order allows.

What "as closely as accumulation order allows" means, measured on this CPU with the restatement itself: the same rounding table with
fp64 instead of fp32 accumulation lands 0.37 x (width 64) / 0.75 x (width 512) of ref_bf16_mean_l1 away from the fp32-accumulation run.
Single one-ulp flips (per layer: ~1e-4 of the outputs) spread through the later layers until they are as large as that; torch's CPU bf16
kernels sum in an order of their own, so no restatement can get closer to wav_ref_bf16 than that floor.  Measured with
weights="module": 0.356 x (w64) and 0.759 x (w512); the bars below are twice that."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from e2e_tts_amd import config as cfgmod, synth_weights as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = {"w64": 0.356, "w512": 0.759}   # restatement (weights="module") vs wav_ref_bf16, in units of ref_bf16_mean_l1


def cfg48(width):
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=width)
    cfg["audio"]["stft"]["hop_length"] = 512
    cfg["audio"]["signal"]["sampling_rate"] = 48000
    return cfg


def mean_l1(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean())


def restate(tag, **kw):
    from bf16_act_ref import Bf16ActVocoder
    g = load_golden("hifigan_48k")
    cfg = cfg48(int(g[f"{tag}.width"]))
    state = sw.make_vocoder_state(cfg, seed=int(g[f"{tag}.weight_seed"]))
    return g, Bf16ActVocoder(state, cfg["models"]["hifigan"], **kw).forward(g[f"{tag}.mel"])


def test_precision_constant_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "e2etts.h")).read()
    m = re.search(r"#define\s+E2ETTS_PRECISION_BF16_ACT\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 3
    from e2e_tts_amd import _lib
    assert _lib.PRECISIONS == {"fp32": 0, "bf16x3": 1, "bf16": 2, "bf16_act": 3}
    for name in ("FP32", "BF16X3", "BF16"):
        v = int(re.search(rf"#define\s+E2ETTS_PRECISION_{name}\s+(\d+)", hdr).group(1))
        assert _lib.PRECISIONS[name.lower()] == v


@pytest.mark.parametrize("tag", ["w64", "w512"])
def test_restatement_reproduces_reference_bf16_run(tag):
    g, wav = restate(tag, weights="module")
    ref16, unit = g[f"{tag}.wav_ref_bf16"], float(g[f"{tag}.ref_bf16_mean_l1"])
    d = mean_l1(wav, ref16) / unit
    print(f"{tag}: restatement (module weights) vs the reference's bf16 run: {d:.3f} x ref_bf16_mean_l1")
    assert d <= 2.0 * MEASURED[tag], d
    # every value is a bf16 value
    assert np.array_equal(torch.from_numpy(wav).bfloat16().float().numpy(), wav)


def test_missing_rounding_point_breaks_the_bar():
    """Leaving out the rounding after c1 + b1 (mode 2's single rounding of bf16(lrelu(c1 + b1))) moves the width-64 generator past the
    bar.  (At width 512 the accumulation-order floor is as large as that difference: only w64 can tell.)"""
    g, wav = restate("w64", weights="module", drop=("c1",))
    d = mean_l1(wav, g["w64.wav_ref_bf16"]) / float(g["w64.ref_bf16_mean_l1"])
    print(f"w64 without the round after c1 + b1: {d:.3f} x")
    assert d > 2.0 * MEASURED["w64"], d


@pytest.mark.parametrize("tag", ["w64", "w512"])
def test_record_engine_weight_path_gap(tag):
    """The engine's parameters (bf16 of the fp32 weight-norm fold) against the module's (weight norm in bf16): the expected extra
    distance from wav_ref_bf16 that the weight path alone causes (printed; the drop-in GPU test allows it as its margin)."""
    g, eng_w = restate(tag, weights="engine")
    _, mod_w = restate(tag, weights="module")
    unit = float(g[f"{tag}.ref_bf16_mean_l1"])
    d_eng, d_mod = mean_l1(eng_w, g[f"{tag}.wav_ref_bf16"]) / unit, mean_l1(mod_w, g[f"{tag}.wav_ref_bf16"]) / unit
    d_fp32 = mean_l1(eng_w, g[f"{tag}.wav"]) / unit
    print(f"{tag}: vs wav_ref_bf16, engine weights {d_eng:.3f} x, module weights {d_mod:.3f} x; engine weights vs fp32 wav {d_fp32:.3f} x")
    assert d_fp32 <= 1.5


def test_accumulation_order_floor():
    """fp32 against fp64 accumulation, same rounding table: the size of what one-ulp flips grow to (the floor quoted above)."""
    g, a = restate("w64", weights="module")
    _, b = restate("w64", weights="module", acc=torch.float64)
    d = mean_l1(a, b) / float(g["w64.ref_bf16_mean_l1"])
    print(f"w64: fp32 vs fp64 accumulation: {d:.3f} x ref_bf16_mean_l1")
    assert 0.0 < d < 2.0 * MEASURED["w64"]
