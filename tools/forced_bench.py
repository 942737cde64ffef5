#!/usr/bin/env python3
"""Times the teacher-forced acoustic pass (e2etts_acoustic_forced) at the headline shape -- B = 32, L = 128, T = 768, default model,
synthetic weights with 6 frames per phoneme -- beside the predicted pass (e2etts_acoustic) of the same session, and the soft-expansion
kernel alone (the engine's event-bracketed profile class "soft_expand": time, and FLOP/s out of 2 B T L H).

The soft map is a smoothed copy of the hard alignment (each frame spreads over its phoneme and both neighbours), the targets are random
frame-resolved arrays; inputs lie in device memory, as after align_audio.  Prints one JSON line.

Usage:  python tools/forced_bench.py [--steps 20] [--warmup 5] [--precision fp32|bf16x3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=128)
    args = ap.parse_args()
    import torch
    from e2e_tts_amd import config as cfgmod, synth_weights as sw
    from e2e_tts_amd.runtime import engine_from_states
    cfg = cfgmod.default_config()
    stats = cfgmod.DEFAULT_STATS
    ac = sw.make_acoustic_state(cfg, stats, 4, seed=1234, mode="fixed")
    voc = sw.make_vocoder_state(cfg, seed=4321)
    eng = engine_from_states(cfg, stats, ac, voc, device=0)
    eng.set_precision("fp32", args.precision)
    B, L, fpp = args.batch, args.length, 6
    T = L * fpp
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    rng = np.random.Generator(np.random.PCG64(1))
    dev = torch.device("cuda", 0)
    ids = torch.from_numpy(rng.integers(4, cfgmod.N_SYMBOLS, (B, L)).astype(np.int64)).to(dev)
    lens = torch.full((B,), L, dtype=torch.int64, device=dev)
    spk = torch.tensor([1], dtype=torch.int64, device=dev)
    dur = torch.full((B, L), float(fpp), dtype=torch.float32, device=dev)
    hard = np.zeros((T, L), np.float32)
    hard[np.arange(T), np.arange(T) // fpp] = 1.0
    soft = 0.6 * hard
    soft[:, 1:] += 0.2 * hard[:, :-1]
    soft[:, :-1] += 0.2 * hard[:, 1:]
    soft /= soft.sum(1, keepdims=True)
    attn = torch.from_numpy(np.broadcast_to(soft, (B, T, L)).copy()).to(dev)
    mel_lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    f0 = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32)).to(dev)
    uv = torch.from_numpy((rng.random((B, T)) > 0.7).astype(np.float32)).to(dev)
    en = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32)).to(dev)
    tg = dict(f0=f0, uv=uv, energy=en, pitch_frames=True, energy_frames=True, T=T, want=())

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        return (time.perf_counter() - t0) / args.steps * 1e3

    res = dict(B=B, L=L, T=T, hidden=H, precision=args.precision, steps=args.steps)
    r = eng.acoustic(ids, lens, spk, want=("mel_lens",))
    assert r["T"] == T, r["T"]
    res["predicted_ms"] = timed(lambda: eng.acoustic(ids, lens, spk, want=()))
    res["forced_soft_ms"] = timed(lambda: eng.acoustic_forced(ids, lens, spk, durations=dur, attn_soft=attn, mel_lens=mel_lens, **tg))
    res["forced_hard_ms"] = timed(lambda: eng.acoustic_forced(ids, lens, spk, durations=dur, **tg))
    res["predicted_again_ms"] = timed(lambda: eng.acoustic(ids, lens, spk, want=()))
    eng.profile_filter("soft_expand")
    eng.profile_enable(True)
    for _ in range(args.steps):
        eng.acoustic_forced(ids, lens, spk, durations=dur, attn_soft=attn, mel_lens=mel_lens, **tg)
    st = [s for s in eng.profile_read() if s["name"] == "soft_expand"]
    eng.profile_enable(False)
    eng.profile_filter(None)
    if st and st[0]["launches"]:
        ms = st[0]["ms"] / st[0]["launches"]
        res.update(soft_expand_us=ms * 1e3, soft_expand_gflop=st[0]["flops"] / st[0]["launches"] / 1e9,
                   soft_expand_tflops=st[0]["flops"] / st[0]["launches"] / (ms * 1e-3) / 1e12)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
