#!/usr/bin/env python3
"""Timing of the vocoder-bias denoiser (csrc/denoiser.hip, include/e2etts.h: e2etts_denoise) on the headline batch of bench.py:
B = 32 utterances of 128 phonemes x 6 frames x 256 samples = 196 608 samples, default config, synthetic weights.

  1. e2etts_denoise alone, audio resident in HBM, result left in HBM: ms per call (torch events around the calls, after a warm-up), and
     per kernel class from the engine's own HIP-event profile: the two conv_gemm launches in TFLOP/s, the three passes in GB/s;
  2. the headline step (e2etts_synthesize, ids in page-locked host memory -> int16 PCM in page-locked host memory) with
     set_denoise(0.1) against set_denoise(0), alternating in one session.
Prints one JSON line at the end.   python tools/denoiser_bench.py [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from e2e_tts_amd import config as cfgmod, denoiser as dn, synth_weights as sw  # noqa: E402
from e2e_tts_amd.runtime import engine_from_states  # noqa: E402

B, PHONEMES, FRAMES_PER_PHONEME = 32, 128, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two settings in part 2")
    args = ap.parse_args()
    cfg, stats = cfgmod.default_config(), cfgmod.DEFAULT_STATS
    ac = sw.make_acoustic_state(cfg, stats, 4, seed=1234, mode="fixed", frames_per_phoneme=FRAMES_PER_PHONEME)
    voc = sw.make_vocoder_state(cfg, seed=4321)
    eng = engine_from_states(cfg, stats, ac, voc, device=0)
    hop = eng.dims.hop_length
    N, H = 1024, 256
    fwd, inv, _ = dn.stft_bases(N, H, N)
    eng.denoiser_load(fwd, inv, N, H)
    bias = eng.denoiser_calibrate(None, 88)
    n = PHONEMES * FRAMES_PER_PHONEME * hop
    rng = np.random.Generator(np.random.PCG64(5))
    audio = torch.from_numpy((0.3 * rng.standard_normal((B, n))).astype(np.float32)).cuda()
    out = torch.empty_like(audio)
    pcm = torch.empty((B, n), dtype=torch.int16, device="cuda")
    res = {"batch": B, "samples_per_utterance": n, "filter_length": N, "hop": H, "bias_l1": float(np.abs(bias).sum())}

    # ---- 1. e2etts_denoise alone
    def call():
        eng.denoise(audio, None, 0.1, out_wav=out, out_pcm=pcm)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    ev[0].record()
    for i in range(args.steps):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
    res["denoise_ms_median"], res["denoise_ms_min"], res["denoise_ms_max"] = statistics.median(per), min(per), max(per)
    eng.profile_filter(None)
    eng.profile_enable(True)
    for _ in range(args.steps):
        call()
    classes = eng.profile_read()
    eng.profile_enable(False)
    res["classes"] = {}
    for st in classes:
        ms = st["ms"] / max(st["launches"], 1)
        rec = {"ms_per_launch": ms, "launches_per_call": st["launches"] / args.steps}
        if st["flops"] > 0:
            rec["tflops"] = st["flops"] / st["launches"] / (ms * 1e-3) / 1e12
        if st["bytes"] > 0:
            rec["gb_per_s"] = st["bytes"] / st["launches"] / (ms * 1e-3) / 1e9
        res["classes"][st["name"]] = rec
        print(f"  {st['name']:32s} {ms:8.3f} ms/launch" + (f"  {rec['tflops']:7.1f} TFLOP/s" if "tflops" in rec else "") +
              (f"  {rec['gb_per_s']:8.0f} GB/s (algorithmic bytes)" if "gb_per_s" in rec else ""), flush=True)
    print(f"e2etts_denoise, {B} x {n} samples: median {res['denoise_ms_median']:.3f} ms (min {res['denoise_ms_min']:.3f}, max {res['denoise_ms_max']:.3f}), "
          f"including the copies in and out of the caller's HBM buffers", flush=True)

    # ---- 2. the headline step with and without the denoiser
    g = np.load(os.path.join(ROOT, "tests", "golden", "bench_b32.npz"), allow_pickle=False)
    ids = torch.from_numpy(np.ascontiguousarray(g["ids"][:B])).pin_memory()
    lens = torch.full((B,), ids.shape[1], dtype=torch.int64).pin_memory()
    spk = torch.ones((1,), dtype=torch.int64).pin_memory()
    T = ids.shape[1] * FRAMES_PER_PHONEME
    hpcm = torch.empty((B, T * hop), dtype=torch.int16).pin_memory()
    hmel = torch.empty((B,), dtype=torch.int64).pin_memory()

    def step():
        return eng.synthesize(ids, lens, spk, out_pcm=hpcm, out_mel_lens=hmel)[2]
    times = {0.0: [], 0.1: []}
    for s in (0.0, 0.1):
        eng.set_denoise(s)
        for _ in range(args.warmup):
            assert step() == T
    for _ in range(args.rounds):
        for s in (0.0, 0.1):
            eng.set_denoise(s)
            step()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()   # synchronous: returns when the PCM is in host memory
            times[s].append((time.perf_counter() - t0) / args.steps * 1e3)
    eng.set_denoise(0.0)
    res["step_ms_denoise_off"], res["step_ms_denoise_on"] = times[0.0], times[0.1]
    res["step_ms_added_median"] = statistics.median(times[0.1]) - statistics.median(times[0.0])
    print(f"headline step, set_denoise(0):   {['%.2f' % t for t in times[0.0]]} ms", flush=True)
    print(f"headline step, set_denoise(0.1): {['%.2f' % t for t in times[0.1]]} ms  (median difference {res['step_ms_added_median']:.2f} ms)", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
