#!/usr/bin/env python3
"""The resampler (libe2etts_resample.so) at the shapes the pipeline has, samples resident in HBM, default filter design.

Steps, each a child process of its own under its own ``timeout`` (a step that fails or runs into its limit ends the run: nothing more
is started on the GPU after it):
  long     (a) 60 s of 48 kHz, B = 1, fp32 -> 8 / 16 / 22.05 kHz: the one-shot call (HIP events around the kernel, e2ers_profile_read:
           median of --repeats calls after --warmup) and the same audio streamed in the vocoder's 512-frame pieces (512 x 512 samples; two
           pushes in flight; wall clock of the whole stream, which includes one launch and one fetch per piece);
  batch    (b) the bench batch's PCM, 32 x 196,608 int16 samples at 22.05 kHz -> 16 / 48 kHz, one-shot;
  c5       BASELINE config 5 (48 kHz generator, 5,632 frames = 60 s, plain bf16, chunks of 512 frames, denoise_strength 0.1) through
           ``Denoiser.stream`` without and with ``output_rate=16000``: wall clock per pass;
  api      ``TTS.inference_ids`` on synthetic full-size checkpoints, 32 sentences, ``output_rate=None`` against ``output_rate=16000``.
For the one-shot calls: milliseconds, effective GB/s of (bytes in + bytes out: fp32 and int16 are both written), GMAC/s.
Prints one JSON line per measurement.  Nothing in the tests depends on these times."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29   # a plain copy on this chip (the microarchitecture guide's measurement): what GB/s figures are set against


def one_shot(a, tag, src, dst, x):
    import torch
    from e2e_tts_amd import resample as rs
    r = rs.Resampler(src, dst, device=0)
    r.profile_enable(True)
    P = -(-r.taps.size // r.L)
    ms, wall = [], []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = r.forward(x, want=())
        w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            ms.append(r.profile_read()["filter"])
            wall.append(w)
    B, n = int(x.shape[0]), int(x.shape[1])
    W = out["width"]
    nbytes = B * n * x.element_size() + B * W * 6
    m = statistics.median(ms)
    rec = dict(step=tag, src=src, dst=dst, L=r.L, M=r.M, taps=int(r.taps.size), P=P, B=B, n=n, n_out=W, tile_outputs=r.tile_outputs, filter_ms=round(m, 4),
               filter_ms_min=round(min(ms), 4), filter_ms_max=round(max(ms), 4), call_wall_ms=round(statistics.median(wall), 4), bytes=nbytes,
               GBps=round(nbytes / m / 1e6, 1), share_of_copy_rate=round(nbytes / m / 1e6 / (COPY_TBPS * 1e3), 4), GMACps=round(B * W * P / m / 1e6, 1),
               device_bytes=r.device_bytes(), repeats=a.repeats)
    print(json.dumps(rec), flush=True)
    return r


def step_long(a):
    import torch
    n = 60 * 48000
    rng = np.random.Generator(np.random.PCG64(3))
    t = np.arange(n) / 48000.0
    x = torch.from_numpy((0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)[None, :]).cuda()
    piece = 512 * 512
    pieces = [x[:, i:i + piece] for i in range(0, n, piece)]
    for dst in (8000, 16000, 22050):
        r = one_shot(a, "long_one_shot", 48000, dst, x)
        times = []
        for i in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            total = sum(p.shape[1] for p in r.stream(pieces))
            times.append((time.perf_counter() - t0) * 1e3)
        assert total == int(r.n_out(n))
        times = times[a.warmup:]
        print(json.dumps(dict(step="long_stream", src=48000, dst=dst, pieces=len(pieces), piece_samples=piece, stream_wall_ms=round(statistics.median(times), 4),
                              stream_wall_ms_min=round(min(times), 4), stream_wall_ms_max=round(max(times), 4), repeats=a.repeats)), flush=True)
        r.close()


def step_batch(a):
    import torch
    rng = np.random.Generator(np.random.PCG64(4))
    x = torch.from_numpy(rng.integers(-20000, 20000, size=(32, 196608), dtype=np.int16)).cuda()
    for dst in (16000, 48000):
        one_shot(a, "batch_one_shot", 22050, dst, x).close()


def step_c5(a):
    from e2e_tts_amd import config as cfgmod, synth_weights as sw
    from e2e_tts_amd.models import Denoiser, HifiGan
    frames, hop = 5632, 512
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=512)
    cfg["audio"]["stft"]["hop_length"] = hop
    cfg["audio"]["signal"]["sampling_rate"] = 48000
    v = HifiGan(cfg["models"]["hifigan"])
    v.load_state_dict(sw.to_torch(sw.make_vocoder_state(cfg, seed=33)))
    v = v.eval().to(0)
    v.engine.set_precision("bf16")
    den = Denoiser(v)
    mel = np.random.Generator(np.random.PCG64(7)).standard_normal((1, frames, 80)).astype(np.float32)
    chunks = [np.ascontiguousarray(mel[:, i:i + 512]) for i in range(0, frames, 512)]
    times = {None: [], 16000: []}
    for i in range(a.warmup + a.repeats):
        for rate in (None, 16000):
            t0 = time.perf_counter()
            total = sum(p.shape[1] for p in den.stream(chunks, strength=0.1, want_pcm=True, output_rate=rate, source_rate=48000))
            if i >= a.warmup:
                times[rate].append((time.perf_counter() - t0) * 1e3)
            assert total == (frames * hop if rate is None else -(-frames * hop // 3))
    rec = dict(step="c5_denoised_stream", frames=frames, chunk_frames=512, repeats=a.repeats)
    for rate, tag in ((None, "plain"), (16000, "to_16k")):
        rec[tag + "_wall_ms"] = round(statistics.median(times[rate]), 3)
        rec[tag + "_wall_ms_range"] = [round(min(times[rate]), 3), round(max(times[rate]), 3)]
    rec["added_ms"] = round(rec["to_16k_wall_ms"] - rec["plain_wall_ms"], 3)
    print(json.dumps(rec), flush=True)


def step_api(a):
    import torch
    import yaml
    from e2e_tts_amd import config as cfgmod, synth_weights as sw
    from e2e_tts_amd.api import TTS
    cfg, stats = cfgmod.default_config(), cfgmod.DEFAULT_STATS
    with tempfile.TemporaryDirectory() as tmp:
        d, v = os.path.join(tmp, "acoustic"), os.path.join(tmp, "vocoder")
        os.makedirs(d)
        os.makedirs(v)
        torch.save({"state_dict": sw.to_torch(sw.make_acoustic_state(cfg, stats, 4, seed=7, mode="varied")), "optimizer": {}}, os.path.join(d, "statedict.pt"))
        torch.save({"state_dict": sw.to_torch(sw.make_vocoder_state(cfg, seed=8))}, os.path.join(v, "statedict.pt"))
        yaml.safe_dump(dict(cfg, train={"seed": 1234}), open(os.path.join(d, "config.yaml"), "w"))
        json.dump(cfgmod.DEFAULT_SPEAKERS, open(os.path.join(d, "speakers.json"), "w"))
        json.dump(stats, open(os.path.join(d, "stats.json"), "w"))
        tts = TTS(os.path.join(d, "statedict.pt"), os.path.join(v, "statedict.pt"), max_len=300, text_to_sequence=lambda t: [4])
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [list(rng.integers(4, 131, int(n))) for n in rng.integers(60, 128, 32)]
    times = {None: [], 16000: []}
    sizes = {}
    for i in range(a.warmup + a.repeats):
        for rate in (None, 16000):
            t0 = time.perf_counter()
            out = tts.inference_ids(seqs, "spk_c", output_rate=rate)
            if i >= a.warmup:
                times[rate].append((time.perf_counter() - t0) * 1e3)
            sizes[rate] = int(out.size)
    rec = dict(step="api_inference_ids", sentences=len(seqs), samples_22k=sizes[None], samples_16k=sizes[16000], repeats=a.repeats)
    for rate, tag in ((None, "plain"), (16000, "to_16k")):
        rec[tag + "_wall_ms"] = round(statistics.median(times[rate]), 3)
        rec[tag + "_wall_ms_range"] = [round(min(times[rate]), 3), round(max(times[rate]), 3)]
    rec["added_ms"] = round(rec["to_16k_wall_ms"] - rec["plain_wall_ms"], 3)
    print(json.dumps(rec), flush=True)


STEPS = {"long": step_long, "batch": step_batch, "c5": step_c5, "api": step_api}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", default="long,batch,c5,api")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds each step may take")
    ap.add_argument("--step", choices=tuple(STEPS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, f"--warmup={a.warmup}", f"--repeats={a.repeats}"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": step, "failed": p.returncode}), flush=True)
            return p.returncode   # nothing more is started after a step that failed or ran into its limit
    return 0


if __name__ == "__main__":
    sys.exit(main())
