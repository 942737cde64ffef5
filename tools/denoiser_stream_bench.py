#!/usr/bin/env python3
"""The denoised vocoder stream (e2etts_vocoder_stream_begin_denoised) on BASELINE config 5 as bench.py runs it: the 48 kHz generator
(upsample 8 x 8 x 4 x 2 = hop 512, width 512), ONE utterance of 5 632 frames = 60.07 s, plain bf16, int16 PCM fetched per chunk, two chunks
in flight; denoiser geometry (1024, 4), bias calibrated on the engine's own vocoder.

  1. chunks of 512 and of 2 048 frames: the stream without and with denoise_strength = 0.1, alternating --rounds times in one session,
     --steps passes each: median and [min, max] ms per pass; per kernel class of one denoised pass from the engine's HIP-event profile;
  2. e2etts_device_bytes before the first stream, after a plain stream and after a denoised stream at chunks of 512, and again after a
     second denoised stream (the slots' workspaces are bounded by the chunk: the figure must not move).
Prints one JSON line at the end.   python tools/denoiser_stream_bench.py [--steps 10] [--rounds 3] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from e2e_tts_amd import config as cfgmod, denoiser as dn, synth_weights as sw  # noqa: E402
from e2e_tts_amd.models import HifiGan  # noqa: E402

FRAMES, HOP = 5632, 512
N, H = 1024, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    cfg = cfgmod.default_config()
    cfg["models"]["hifigan"].update(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=512)
    cfg["audio"]["stft"]["hop_length"] = HOP
    cfg["audio"]["signal"]["sampling_rate"] = 48000
    v = HifiGan(cfg["models"]["hifigan"])
    v.load_state_dict(sw.to_torch(sw.make_vocoder_state(cfg, seed=33)))
    eng = v.eval().to(0).engine
    eng.set_precision("bf16")
    fwd, inv, _ = dn.stft_bases(N, H, N)
    eng.denoiser_load(fwd, inv, N, H)
    eng.denoiser_calibrate(None, 88)
    mel = np.random.Generator(np.random.PCG64(7)).standard_normal((1, FRAMES, 80)).astype(np.float32)
    res = {"frames": FRAMES, "hop_length": HOP, "filter_length": N, "hop": H, "delay_frames": dn.stream_delay_frames(N, H, HOP), "chunks": {}}
    bytes_ = {"before": eng.device_bytes()}

    for chunk in (512, 2048):
        chunks = [np.ascontiguousarray(mel[:, i:i + chunk]) for i in range(0, FRAMES, chunk)]

        def run(strength):
            return sum(p.shape[1] for p in eng.vocoder_stream(chunks, 1, want_pcm=True, denoise_strength=strength))
        for s in (None, 0.1):
            for _ in range(args.warmup):
                assert run(s) == FRAMES * HOP
            if chunk == 512:
                bytes_["after_plain_stream" if s is None else "after_denoised_stream"] = eng.device_bytes()
        times = {None: [], 0.1: []}
        for _ in range(args.rounds):
            for s in (None, 0.1):
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    run(s)
                    times[s].append((time.perf_counter() - t0) * 1e3)
        if chunk == 512:
            bytes_["after_more_denoised_streams"] = eng.device_bytes()
        rec = {}
        for s, tag in ((None, "plain"), (0.1, "denoised")):
            rec[tag] = {"ms_median": statistics.median(times[s]), "ms_min": min(times[s]), "ms_max": max(times[s]),
                        "round_medians": [statistics.median(times[s][r * args.steps:(r + 1) * args.steps]) for r in range(args.rounds)]}
            print(f"chunks of {chunk:4d}: {tag:8s} median {rec[tag]['ms_median']:.3f} ms [{rec[tag]['ms_min']:.3f}, {rec[tag]['ms_max']:.3f}]  "
                  f"per round {['%.3f' % t for t in rec[tag]['round_medians']]}", flush=True)
        rec["added_ms_median"] = rec["denoised"]["ms_median"] - rec["plain"]["ms_median"]
        eng.profile_filter(None)
        eng.profile_enable(True)
        run(0.1)
        classes = eng.profile_read()
        eng.profile_enable(False)
        rec["denoiser_classes_ms_per_pass"] = {st["name"]: {"ms": st["ms"], "launches": st["launches"]} for st in classes
                                               if st["name"].startswith(("dn_", "denoise_"))}
        rec["all_classes_ms_per_pass"] = sum(st["ms"] for st in classes)
        for name, c in rec["denoiser_classes_ms_per_pass"].items():
            print(f"    {name:32s} {c['ms']:7.3f} ms in {c['launches']} launches per pass", flush=True)
        print(f"    denoiser kernels {sum(c['ms'] for c in rec['denoiser_classes_ms_per_pass'].values()):.3f} ms of {rec['all_classes_ms_per_pass']:.3f} ms "
              f"of kernels per pass (profiled: slots serialised); wall-clock difference {rec['added_ms_median']:.3f} ms", flush=True)
        res["chunks"][str(chunk)] = rec
    res["device_bytes"] = bytes_
    print("e2etts_device_bytes:", bytes_, flush=True)
    print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
