#!/usr/bin/env python3
"""The pitch tracker (libe2etts_f0.so) at the pipeline's two shapes, samples resident in HBM:
  batch   32 rows of 8.9 s at 22.05 kHz, hop 256 (767 frames a row): forward and targets, and the mel front-end's forward on the same
          batch (the figure tools/mel_bench.py reports at its 768-frame shape) beside them;
  long    one 60 s row at 48 kHz, hop 512 (5625 frames).
Each step is a child process of its own under its own ``timeout`` (a step that fails or runs into its limit ends the run: nothing more is
started on the GPU after it).  The phases {analyse, path, targets} are timed with HIP events (e2ef0_profile_read), repeated after
--warmup calls until --fill-seconds of wall clock are filled; medians and [min, max].  Prints one JSON line per step.  Nothing in the
tests depends on these times."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def recordings(B, n, sr, seed=3):
    """Voiced stretches (a five-harmonic tone with vibrato, a pitch of its own per row) with pauses of low noise: float32 [B, n]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)[None, :] / float(sr)
    f0 = rng.uniform(90, 350, (B, 1)) * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(f0, 1) / sr
    x = sum(a * np.sin((k + 1) * ph) for k, a in enumerate((1.0, 0.5, 0.35, 0.2, 0.1))) * 0.15
    gate = np.sin(2 * np.pi * 0.8 * t + rng.uniform(0, 6.28, (B, 1))) > -0.5
    return np.clip(x * gate + 0.003 * rng.standard_normal((B, n)), -1, 1).astype(np.float32)


def measure(a, tag, B, n, sr, hop, with_mel):
    import torch
    from e2e_tts_amd import config as cfgmod, f0 as f0lib
    x = torch.from_numpy(recordings(B, n, sr)).cuda()
    torch.cuda.synchronize()
    trk = f0lib.PitchTracker(sr, hop)
    trk.profile_enable(True)
    fe = None
    if with_mel:
        from e2e_tts_amd import mel as mp
        fe = mp.MelFrontend(1024, hop, 80, device=0)
        fe.load(mp.dft_basis(1024), mp.mel_filterbank(sr, 1024, 80, 0.0, 8000.0))
        fe.profile_enable(True)
    ms = {"analyse": [], "path": [], "targets": [], "forward_wall": [], "mel_phases": []}
    t_begin, i = time.perf_counter(), 0
    while i < a.warmup + 3 or (time.perf_counter() - t_begin < a.fill_seconds and i < 2000):
        t0 = time.perf_counter()
        r = trk.forward(x, want=())
        wall = (time.perf_counter() - t0) * 1e3
        trk.targets(cfgmod.DEFAULT_STATS, fetch=False)
        p = trk.profile_read()
        mel_ms = None
        if fe is not None:
            fe.forward(x, want=())
            mel_ms = sum(fe.profile_read().values())
        if i >= a.warmup:
            for k in ("analyse", "path", "targets"):
                ms[k].append(p[k])
            ms["forward_wall"].append(wall)
            if mel_ms is not None:
                ms["mel_phases"].append(mel_ms)
        i += 1
    f0 = trk.forward(x)["f0"]
    rec = dict(step=tag, B=B, samples=n, sample_rate=sr, hop=hop, T=r["T"], W=trk.W, lags=trk.lags, tile_frames=trk.tile_frames, repeats=len(ms["analyse"]),
               voiced_share=round(float((f0 > 0).mean()), 3), device_bytes=trk.device_bytes())
    mac = float(B) * r["T"] * ((trk.W + 3) // 4 * 4) * ((trk.lags + 3) // 4 * 4)
    for k, v in ms.items():
        if v:
            rec[k + "_ms"], rec[k + "_ms_range"] = round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]
    rec["lag_gmac"] = round(mac / 1e9, 2)
    rec["analyse_TFLOPs"] = round(2 * mac / rec["analyse_ms"] / 1e9, 2)
    print(json.dumps(rec), flush=True)
    trk.close()


def step_batch(a):
    measure(a, "batch_32x8.9s_22k", 32, int(8.9 * 22050), 22050, 256, True)


def step_long(a):
    measure(a, "long_60s_48k", 1, 60 * 48000, 48000, 512, False)


STEPS = {"batch": step_batch, "long": step_long}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fill-seconds", type=float, default=1.0, help="repeats go on until this much wall clock is filled")
    ap.add_argument("--steps", default="batch,long")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds each step may take")
    ap.add_argument("--step", choices=tuple(STEPS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, f"--warmup={a.warmup}",
               f"--fill-seconds={a.fill_seconds}"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": step, "failed": p.returncode}), flush=True)
            return p.returncode   # nothing more is started after a step that failed or ran into its limit
    return 0


if __name__ == "__main__":
    sys.exit(main())
