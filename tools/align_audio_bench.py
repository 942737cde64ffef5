#!/usr/bin/env python3
"""Wall time of models.UnsupervisedFastSpeech2.align_audio at the aligner bench shape (B = 32, L = 128, T = 768 frames of 256 samples)
with the beta-binomial prior built on the host (attn_prior=None: scipy, then an upload) and generated on the device
(attn_prior="device").  The model is the tiny configuration (hidden 64, n_mel 80) with synthetic weights: the prior's cost depends on
(B, T, L) alone.  Prints one JSON line; asserts the gate that the device prior is the faster of the two."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--T", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from e2e_tts_amd import config as cfgmod, synth_weights as sw
    from e2e_tts_amd.models import UnsupervisedFastSpeech2
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=3, mode="varied")
    m = UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, 80, fs, cfgmod.DEFAULT_STATS, device=0)
    m.load_state_dict(sw.to_torch(state))
    B, L, T = a.B, a.L, a.T
    hop = m._default_stft().frontend.hop
    rng = np.random.Generator(np.random.PCG64(3))
    txt_lens = rng.integers(L // 2, L + 1, B).astype(np.int64)
    wav_lens = rng.integers(T // 2, T + 1, B).astype(np.int64) * hop
    txt_lens[0], wav_lens[0] = L, T * hop
    ids = torch.from_numpy(rng.integers(1, cfgmod.N_SYMBOLS, (B, L)))
    wavs = torch.from_numpy((rng.standard_normal((B, T * hop)) * 0.1).astype(np.float32)).cuda()
    spk = torch.from_numpy(rng.integers(0, 4, B))
    out = {"B": B, "L": L, "T": T, "repeats": a.repeats}
    durs = {}
    for name, prior in (("none", None), ("device", "device")):
        ms = []
        for i in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = m.align_audio(spk, ids, txt_lens, wavs, wav_lens, attn_prior=prior)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[f"align_audio_{name}_ms"] = round(statistics.median(ms), 3)
        durs[name] = r[2].cpu().numpy()
    out["rows_with_equal_durations"] = int(sum(np.array_equal(durs["none"][b], durs["device"][b]) for b in range(B)))
    out["speedup"] = round(out["align_audio_none_ms"] / out["align_audio_device_ms"], 1)
    print(json.dumps(out), flush=True)
    assert out["align_audio_device_ms"] < out["align_audio_none_ms"], "attn_prior='device' must be faster than attn_prior=None"


if __name__ == "__main__":
    main()
