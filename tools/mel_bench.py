#!/usr/bin/env python3
"""The mel front-end at the bench shape: B = 32 rows of 768 * 256 samples, n_fft 1024 / hop 256 / 80 mels, samples resident in HBM.

Three steps, each a child process of its own under its own ``timeout`` (a step that fails or runs into its limit ends the run: nothing
more is started on the GPU after it):
  hip        e2emel_forward: HIP-event times of {pad, transform, tail} and the wall time of the whole call (it returns after the handle's
             stream has drained), median of --repeats calls after --warmup; the tail's achieved GB/s over the bytes it reads and writes
             (the spectrum rows of real frames once, mel and energy once), the transform's TFLOP/s, device memory held;
  torch_gpu  the same formula as plain PyTorch ops on the same GPU (the restatement of tests/mel_ref.py in torch: reflect pad, unfold,
             one matmul with the same DFT basis, the elementwise tail, one matmul with the filterbank), timed with torch events;
  torch_cpu  the same ops on --cpus CPU threads.
Prints one JSON line per step and one summary line.  Nothing in the tests depends on these times."""
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


def make_audio(B, n, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)[None, :] / 22050.0
    f0 = rng.uniform(100, 400, (B, 1))
    x = 0.4 * np.sin(2 * np.pi * f0 * t) + 0.1 * rng.standard_normal((B, n))
    return np.clip(x, -1, 1).astype(np.float32)


def torch_formula(torch, x, dft, basis, n_fft, hop, clip=1e-5):
    """tests/mel_ref.py in torch ops: [B, n] -> (log-mel [B, T, n_mel], energy [B, T])."""
    half = (n_fft - hop) // 2
    bins = n_fft // 2 + 1
    y = torch.nn.functional.pad(x[:, None, :], (half, half), mode="reflect")[:, 0]
    fr = y.unfold(1, n_fft, hop)                         # [B, T, n_fft]
    spec = fr @ dft.T                                    # [B, T, 2 bins]
    re, im = spec[..., :bins], spec[..., bins:]
    mag = torch.sqrt((re * re + im * im) + 1e-9)
    mel = torch.log(torch.clamp(mag @ basis.T, min=clip))
    return mel, torch.sqrt((mag * mag).sum(-1))


def step_hip(a):
    import torch
    from e2e_tts_amd import mel as mp
    B, n = a.B, a.frames * a.hop
    fe = mp.MelFrontend(a.n_fft, a.hop, a.n_mel, device=0)
    fe.load(mp.dft_basis(a.n_fft), mp.mel_filterbank(22050, a.n_fft, a.n_mel, 0.0, 8000.0))
    fe.profile_enable(True)
    x = torch.from_numpy(make_audio(B, n)).cuda()
    torch.cuda.synchronize()
    rows = {"pad": [], "transform": [], "tail": [], "call_wall": []}
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        r = fe.forward(x, want=())
        wall = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            ms = fe.profile_read()
            for k in ("pad", "transform", "tail"):
                rows[k].append(ms[k])
            rows["call_wall"].append(wall)
    out = {f"{k}_ms": round(statistics.median(v), 4) for k, v in rows.items()}
    T, bins = r["T"], a.n_fft // 2 + 1
    cpad = (2 * bins + 31) // 32 * 32
    R = T + a.n_fft // a.hop - 1
    tail_bytes = B * T * (2 * bins + a.n_mel + 1) * 4
    flop = 2.0 * B * R * cpad * a.n_fft
    out.update(step="hip", B=B, T=T, n_fft=a.n_fft, hop=a.hop, n_mel=a.n_mel, repeats=a.repeats, tile_frames=fe.tile_frames, device_bytes=fe.device_bytes(),
               tail_bytes=tail_bytes, tail_GBps=round(tail_bytes / out["tail_ms"] / 1e6, 1), transform_gflop=round(flop / 1e9, 2),
               transform_TFLOPs=round(flop / out["transform_ms"] / 1e9, 1), phases_ms=round(out["pad_ms"] + out["transform_ms"] + out["tail_ms"], 4))
    # what the comparison steps check themselves against
    mel = np.empty((B, T, a.n_mel), np.float32)
    fe.forward(x, out_mel=mel, want=())
    os.makedirs(a.scratch, exist_ok=True)
    np.save(os.path.join(a.scratch, "mel_bench_hip_row0.npy"), mel[0])
    print(json.dumps(out), flush=True)


def step_torch(a, gpu):
    import torch
    from e2e_tts_amd import mel as mp
    torch.set_grad_enabled(False)
    if not gpu:
        torch.set_num_threads(a.cpus)
    dev = torch.device("cuda" if gpu else "cpu")
    B, n = a.B, a.frames * a.hop
    x = torch.from_numpy(make_audio(B, n)).to(dev)
    dft = torch.from_numpy(mp.dft_basis(a.n_fft)).to(dev)
    basis = torch.from_numpy(mp.mel_filterbank(22050, a.n_fft, a.n_mel, 0.0, 8000.0)).to(dev)
    repeats, warmup = (a.repeats, a.warmup) if gpu else (max(3, a.repeats // 10), 1)
    times = []
    for i in range(warmup + repeats):
        if gpu:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mel, energy = torch_formula(torch, x, dft, basis, a.n_fft, a.hop)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
        else:
            t0 = time.perf_counter()
            mel, energy = torch_formula(torch, x, dft, basis, a.n_fft, a.hop)
            ms = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            times.append(ms)
    out = dict(step="torch_gpu" if gpu else "torch_cpu", ms=round(statistics.median(times), 3), repeats=repeats)
    if not gpu:
        out["cpus"] = a.cpus
    p = os.path.join(a.scratch, "mel_bench_hip_row0.npy")
    if os.path.exists(p):
        out["mean_abs_diff_vs_hip_row0"] = float(np.abs(mel[0].cpu().numpy() - np.load(p)).mean())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--frames", type=int, default=768)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--n-mel", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds each step may take")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "mel_bench"))
    ap.add_argument("--step", choices=("hip", "torch_gpu", "torch_cpu"), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.step:
        return step_hip(a) if a.step == "hip" else step_torch(a, a.step == "torch_gpu")
    results = {}
    for step in ("hip", "torch_gpu") + (() if a.no_cpu else ("torch_cpu",)):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step] + [
            f"--{k}={getattr(a, k.replace('-', '_'))}" for k in ("B", "frames", "n-fft", "hop", "n-mel", "warmup", "repeats", "cpus", "scratch")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": step, "failed": p.returncode}), flush=True)
            return p.returncode   # nothing more is started after a step that failed or ran into its limit
        results[step] = json.loads(p.stdout.strip().splitlines()[-1])
    h = results["hip"]
    summary = dict(summary=True, hip_call_wall_ms=h["call_wall_ms"], hip_phases_ms=h["phases_ms"], torch_gpu_ms=results["torch_gpu"]["ms"],
                   torch_gpu_over_hip=round(results["torch_gpu"]["ms"] / h["phases_ms"], 2))
    if "torch_cpu" in results:
        summary.update(torch_cpu_ms=results["torch_cpu"]["ms"], torch_cpu_over_hip=round(results["torch_cpu"]["ms"] / h["phases_ms"], 1))
    print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
