#!/usr/bin/env python3
"""Recording conditioning (libe2etts_condition.so) at two shapes, samples resident in HBM:
  batch   32 x 10 s of 44.1 kHz stereo: downmix, analyze (trim="reference"), apply (int16 out) at -20 dBFS;
  long    one 10-minute mono recording at 44.1 kHz: analyze and apply.
Each step is a child process of its own under its own ``timeout`` (a step that fails or runs into its limit ends the run: nothing more is
started on the GPU after it).  The device passes are timed with HIP events (e2econd_profile_read, the "compute" phase of each call),
repeated until a second of wall clock is filled, and alternate in the same process with the CPU path: the same steps through the standard
library's audioop as pydub drives it (tomono, rms per 1 ms step, mul), --cpu-repeats times.  Per pass: milliseconds, the bytes it has to
move (samples read + samples written) and that rate against the 6.29 TB/s a plain copy reaches on this chip.
Prints one JSON line per measurement.  Nothing in the tests depends on these times."""
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

COPY_TBPS = 6.29   # a plain copy on this chip (the microarchitecture guide's measurement): what GB/s figures are set against
RATE, TARGET = 44100, -20.0


def recording(n, seed):
    """Room tone, speech-like noise with pauses, room tone: int16 [n]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(-6000, 6001, n).astype(np.int16)
    ms = RATE // 1000
    x[:300 * ms] = rng.integers(-30, 31, 300 * ms)
    x[n - 200 * ms:] = rng.integers(-30, 31, 200 * ms)
    for a in range(2000 * ms, n - 1000 * ms, 3000 * ms):   # a 250 ms pause every 3 s
        x[a:a + 250 * ms] = rng.integers(-30, 31, 250 * ms)
    return x


def cpu_path(rows, stereo):
    """The audioop path on the same recordings -> seconds (None without audioop)"""
    try:
        import audioop
    except ImportError:
        return None
    import math
    t0 = time.perf_counter()
    thresh = 10 ** (-50 / 20) * 32768
    for row in rows:
        data = row.tobytes()
        if stereo:
            data = audioop.tomono(data, 2, 0.5, 0.5)
        n = len(data) // 2
        L = round(1000 * (n / RATE))
        pos = lambda p: int(p * (RATE / 1000.0))   # noqa: E731
        starts = [i for i in range(L - 100 + 1) if audioop.rms(data[2 * pos(i):2 * pos(i + 100)], 2) <= thresh]
        s = 0
        if starts and starts[0] == 0:
            prev = 0
            for i in starts[1:]:
                if i > prev + 100:
                    break
                prev = i
            s = prev + 100
        kept = data[2 * pos(s):2 * pos(L)]
        r = audioop.rms(kept, 2)
        audioop.mul(kept, 2, 10 ** ((TARGET - 20 * math.log(r / 32768, 10)) / 20) if r else 1.0)
    return time.perf_counter() - t0


def measure(a, tag, rows, stereo):
    import torch
    from e2e_tts_amd import condition as cd
    B, n = len(rows), len(rows[0]) // (2 if stereo else 1)   # frames
    x = torch.from_numpy(np.stack(rows)).cuda()
    lens = np.full(B, n, np.int64)
    c = cd.Conditioner(RATE)
    c.profile_enable(True)
    ms = {"downmix": [], "analyze": [], "apply": []}
    cpu = []
    t_begin, i = time.perf_counter(), 0
    while i < a.warmup + 3 or (time.perf_counter() - t_begin < a.fill_seconds and i < 2000):
        src = x
        if stereo:
            c.downmix(x, fetch=False)
            d = c.profile_read()["compute"]
            src = c.resident_mono()
        r = c.analyze(src, lens, "reference")
        an = c.profile_read()["compute"]
        gain = np.array([cd.loudness_gain(int(s), int(k), TARGET) for s, k in zip(r["sumsq"], r["n_out"])])
        c.apply(gain, want=("pcm",), fetch=False)
        ap = c.profile_read()["compute"]
        if i >= a.warmup:
            if stereo:
                ms["downmix"].append(d)
            ms["analyze"].append(an)
            ms["apply"].append(ap)
        if i < a.cpu_repeats:   # the CPU path, alternating with the device's in the same process
            t = cpu_path(rows, stereo)
            if t is not None:
                cpu.append(t * 1e3)
            t_begin += t or 0.0   # (the second to fill is the device's)
        i += 1
    kept = int(r["n_out"].sum())
    moved = {"downmix": B * n * 6, "analyze": B * n * 2, "apply": kept * 4}
    rec = dict(step=tag, B=B, frames=n, stereo=stereo, rate=RATE, repeats=len(ms["analyze"]), ranges_row0=len(r["ranges"][0]), kept_samples=kept, device_bytes=c.device_bytes())
    total = 0.0
    for k, v in ms.items():
        if not v:
            continue
        m = statistics.median(v)
        total += m
        rec[k + "_ms"], rec[k + "_ms_range"] = round(m, 4), [round(min(v), 4), round(max(v), 4)]
        rec[k + "_bytes"], rec[k + "_GBps"] = moved[k], round(moved[k] / m / 1e6, 1)
        rec[k + "_share_of_copy_rate"] = round(moved[k] / m / 1e6 / (COPY_TBPS * 1e3), 4)
    rec["device_total_ms"] = round(total, 4)
    if cpu:
        rec["audioop_ms"], rec["audioop_repeats"] = round(statistics.median(cpu), 1), len(cpu)
    print(json.dumps(rec), flush=True)
    c.close()


def step_batch(a):
    rows = [np.stack([recording(10 * RATE, 100 + b), recording(10 * RATE, 200 + b)], 1).reshape(-1) for b in range(32)]
    measure(a, "batch_32x10s_stereo", rows, True)


def step_long(a):
    measure(a, "long_10min_mono", [recording(600 * RATE, 7)], False)


STEPS = {"batch": step_batch, "long": step_long}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fill-seconds", type=float, default=1.0, help="device repeats go on until this much wall clock is filled")
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--steps", default="batch,long")
    ap.add_argument("--step-timeout", type=int, default=200, help="seconds each step may take")
    ap.add_argument("--step", choices=tuple(STEPS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, f"--warmup={a.warmup}",
               f"--fill-seconds={a.fill_seconds}", f"--cpu-repeats={a.cpu_repeats}"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": step, "failed": p.returncode}), flush=True)
            return p.returncode   # nothing more is started after a step that failed or ran into its limit
    return 0


if __name__ == "__main__":
    sys.exit(main())
