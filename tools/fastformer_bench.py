#!/usr/bin/env python3
"""Acoustic-model step time with FFT blocks ("transformer") and with Fastformer blocks ("fastformer"), full-size model, exact fp32,
on the same GPU and build, interleaved.  (bench.py's --blocks has fixed choices; correctness of the block: tests/test_gpu_fastformer.py.)

Shapes: the headline batch (B = 32, L = 128 phonemes, 6 frames each -> T = 768), B = 1 of the same length, and the long-form shape
B = 1, L = 512 -> T = 3072, where the FFT block's attention is quadratic in T and the Fastformer's pooling linear.

Per shape: wall time of Engine.acoustic (host clock around a call that ends in a device synchronise; median and min of --reps calls
after --warmup, the two block types alternating call by call), then ONE more call per block type under the engine's event profile:
per-class kernel times, and for `ff_pool` the fraction of HBM bandwidth it reaches -- it reads [B, N, H] once, that is its roof
(8.0 TB/s spec; a float4 copy reaches 6.3 TB/s on this part).

    python tools/fastformer_bench.py [--reps 20] [--warmup 5] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from e2e_tts_amd import config as cfgmod, synth_weights as sw  # noqa: E402

HBM_SPEC = 8.0e12
SHAPES = (("headline B=32 L=128 T=768", 32, 128), ("B=1 L=128 T=768", 1, 128), ("long B=1 L=512 T=3072", 1, 512))
ATTENTION_CLASSES = {"transformer": ("attention",), "fastformer": ("ff_pool", "ff_scale")}


def make_engine(block):
    from e2e_tts_amd.runtime import engine_from_states
    cfg = cfgmod.default_config()
    cfg["models"]["fastspeech2"]["building_block"]["block_type"] = block
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=1234, mode="fixed", frames_per_phoneme=6)
    eng = engine_from_states(cfg, cfgmod.DEFAULT_STATS, ac, sw.make_vocoder_state(cfg, seed=4321), device=0)
    eng.set_precision("fp32", "fp32")
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    blocks = ("transformer", "fastformer")
    engines = {b: make_engine(b) for b in blocks}
    rng = np.random.Generator(np.random.PCG64(5))
    spk = np.array([1], np.int64)
    results = []
    for label, B, L in SHAPES:
        ids = rng.integers(4, 131, size=(B, L)).astype(np.int64)
        lens = np.full((B,), L, np.int64)
        times = {b: [] for b in blocks}
        T = None
        for i in range(args.warmup + args.reps):
            for b in blocks:   # alternating: both see the same neighbours on a shared host
                t0 = time.perf_counter()
                r = engines[b].acoustic(ids, lens, spk, want=("mel_lens",))
                dt = time.perf_counter() - t0
                T = r["T"]
                if i >= args.warmup:
                    times[b].append(dt)
        row = dict(shape=label, B=B, L=L, T=int(T))
        print(f"== {label} (T = {T}), fp32, {args.reps} calls each, alternating")
        for b in blocks:
            ts = sorted(times[b])
            row[b] = dict(median_ms=ts[len(ts) // 2] * 1e3, min_ms=ts[0] * 1e3, max_ms=ts[-1] * 1e3)
            print(f"   {b:12s} acoustic(): median {row[b]['median_ms']:8.3f} ms   min {row[b]['min_ms']:8.3f}   max {row[b]['max_ms']:8.3f}", flush=True)
        for b in blocks:   # one profiled call (events around every launch serialise the stream: class times, not a step time)
            eng = engines[b]
            eng.profile_filter(None)
            eng.profile_enable(True)
            eng.profile_read()
            eng.acoustic(ids, lens, spk, want=("mel_lens",))
            eng.sync()
            st = eng.profile_read()
            eng.profile_enable(False)
            tot = sum(s["ms"] for s in st)
            att = sum(s["ms"] for s in st if s["name"] in ATTENTION_CLASSES[b])
            row[b]["classes"] = {s["name"]: dict(launches=s["launches"], ms=s["ms"], bytes=s.get("bytes", 0.0), flops=s["flops"]) for s in st}
            row[b]["attention_ms"] = att
            print(f"   {b}: {tot:.3f} ms of kernel time in one profiled call; attention part ({', '.join(ATTENTION_CLASSES[b])}): {att:.3f} ms")
            for s in sorted(st, key=lambda s: -s["ms"]):
                line = f"      {s['name']:24s} {s['launches']:4d} launches {s['ms']:8.3f} ms  {s['ms'] / max(s['launches'], 1) * 1e3:8.1f} us each"
                if s["name"] == "ff_pool" and s.get("bytes"):
                    bw = s["bytes"] / (s["ms"] * 1e-3)
                    row[b]["ff_pool_hbm_fraction"] = bw / HBM_SPEC
                    line += f"  {bw / 1e12:6.3f} TB/s of input = {100 * bw / HBM_SPEC:5.1f} % of the 8 TB/s HBM spec"
                print(line, flush=True)
        results.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
