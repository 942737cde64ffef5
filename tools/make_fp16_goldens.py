#!/usr/bin/env python3
"""Generate tests/golden/hifigan_fp16.npz by running the REFERENCE's own HifiGan class on CPU in fp32 and after .half().

The fixture pins the vocoder precision "fp16_act" (E2ETTS_PRECISION_FP16_ACT, include/e2etts.h): per case it holds the channels-last mel,
the reference's fp32 wav, the wav of the same module after .half() on mel.half() (wav_ref_fp16, stored as float16: exact), the mean-L1
between the two (ref_fp16_mean_l1: the unit the tests measure in), the weight seed and the geometry.

  48k_w512   BASELINE config 5's generator (rates [8, 8, 4, 2], width 512), B = 1, T = 90 -- the mel and weights of hifigan_48k's w512
  22k_v1     the shipped 22 kHz V1 generator, B = 2, T = 40
  22k_rb2    the same with ResBlock2
  shallow    width 64, one upsampler (rate 2, kernel 4), one ResBlock1 of kernel 3 and dilations (1, 3, 5), B = 2, T = 300: so few layers
             that accumulation-order flips stay small and a missing rounding point shows (tests/test_fp16_act_host.py)

Reference import as in oracle/make_goldens.py (imported from there, not copied).

Usage:  python tools/make_fp16_goldens.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from e2e_tts_amd import config as cfgmod, synth_weights as sw  # noqa: E402
from oracle.make_goldens import GOLD, import_reference  # noqa: E402

# tag -> (hifigan overrides, B, T, weight seed, mel seed)
CASES = {
    "48k_w512": (dict(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=512), 1, 90, 34, 8),
    "22k_v1": (dict(), 2, 40, 41, 21),
    "22k_rb2": (dict(resblock=2, resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]]), 1, 48, 42, 22),
    "shallow": (dict(upsample_rates=[2], upsample_kernel_sizes=[4], upsample_initial_channel=64, resblock_kernel_sizes=[3],
                     resblock_dilation_sizes=[[1, 3, 5]]), 2, 300, 51, 61),
}
GEOMETRY_KEYS = ("resblock", "upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock_kernel_sizes",
                 "resblock_dilation_sizes")


def config_for(overrides: dict) -> dict:
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(overrides)
    hop = int(np.prod(cfg["models"]["hifigan"]["upsample_rates"]))
    cfg["audio"]["stft"]["hop_length"] = hop
    if hop == 512:
        cfg["audio"]["signal"]["sampling_rate"] = 48000
    return cfg


def main():
    import torch
    models = import_reference()
    torch.set_grad_enabled(False)
    arrays = {}
    for tag, (over, B, T, wseed, mseed) in CASES.items():
        cfg = config_for(over)
        hg = cfg["models"]["hifigan"]
        hop = cfg["audio"]["stft"]["hop_length"]
        state = sw.make_vocoder_state(cfg, seed=wseed)
        v = models.HifiGan(hg)
        v.load_state_dict(sw.to_torch(state), strict=True)
        v.eval()
        mel = np.random.Generator(np.random.PCG64(mseed)).standard_normal((B, T, 80)).astype(np.float32)   # channels-last, as the engine takes it
        x = torch.from_numpy(np.ascontiguousarray(mel.transpose(0, 2, 1)))
        peak = [0.0]
        hooks = [m.register_forward_hook(lambda mod, i, o: peak.__setitem__(0, max(peak[0], float(o.abs().max()))))
                 for m in v.modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d))]
        wav = v(x).squeeze(1).numpy()
        for h in hooks:
            h.remove()
        assert wav.shape == (B, T * hop), wav.shape
        wav16 = copy.deepcopy(v).half()(x.half()).squeeze(1)
        assert wav16.dtype == torch.float16 and tuple(wav16.shape) == wav.shape and bool(torch.isfinite(wav16).all())
        wav16 = wav16.numpy()
        unit = float(np.abs(wav16.astype(np.float64) - wav.astype(np.float64)).mean())
        sub = float(((np.abs(wav16) < 2.0 ** -14) & (wav16 != 0)).mean())
        print(f"[{tag}] B={B} T={T} hop={hop}: .half() vs fp32 wav mean-L1 {unit:.3e}; largest layer output (fp32 run) {peak[0]:.2f}; "
              f"subnormal output samples {100 * sub:.3f} %", flush=True)
        arrays[f"{tag}.mel"] = mel
        arrays[f"{tag}.wav"] = wav.copy()
        arrays[f"{tag}.wav_ref_fp16"] = wav16.copy()
        arrays[f"{tag}.ref_fp16_mean_l1"] = np.float64(unit)
        arrays[f"{tag}.weight_seed"] = np.int64(wseed)
        arrays[f"{tag}.mel_seed"] = np.int64(mseed)
        arrays[f"{tag}.hop"] = np.int64(hop)
        for k in GEOMETRY_KEYS:
            arrays[f"{tag}.{k}"] = np.asarray(hg[k], np.int64)
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "hifigan_fp16.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1024:.0f} KiB)", flush=True)
    assert size < 1 << 20, f"{path} is {size} bytes: committed files stay under 1 MiB"


if __name__ == "__main__":
    main()
