#!/usr/bin/env python3
"""Forced alignment at the bench batch: B = 32, L = 128, T = 768 with the shipped widths (hidden 384, n_mel 80), inputs resident in HBM.

Records (median over --repeats calls after --warmup): HIP-event times of the projections, the attention pass and the search inside one
e2ealign_align call, the wall time of the whole call (it returns after the handle's stream has drained), the handle's device memory next to
the size of one [B, T, L] map and of the reference's [B, n_att, T, L] tensor, and, for scale, the plain-loop numpy search of
tests/aligner_ref.py over the same batch on --cpus processes.  Prints one JSON line.  Nothing in the tests depends on these times.

--prior says where the beta-binomial prior comes from: ``given`` (built before the loop and resident in HBM: e2ealign_align), ``device``
(generated inside the attention pass: e2ealign_align_bb) or ``host`` (aligner.batch_prior, scipy, and its upload INSIDE the timed loop,
reported as host_prior_ms: what attn_prior=None costs a caller per batch)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _cpu_mas(args):
    import aligner_ref as ar
    attn, n, m = args
    return ar.mas_loops(attn[:m, :n]).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--T", type=int, default=768)
    ap.add_argument("--hidden", type=int, default=384)
    ap.add_argument("--n-mel", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--prior", choices=("given", "device", "host"), default="given")
    a = ap.parse_args()
    import torch
    from e2e_tts_amd import aligner as al, packer, synth_weights as sw
    B, L, T, H, M = a.B, a.L, a.T, a.hidden, a.n_mel
    rng = np.random.Generator(np.random.PCG64(3))
    state = sw.make_aligner_state(H, M, seed=77)
    txt_lens = rng.integers(L // 2, L + 1, B).astype(np.int64)
    mel_lens = rng.integers(T // 2, T + 1, B).astype(np.int64)
    txt_lens[0], mel_lens[0] = L, T
    ids = rng.integers(1, state["encoder.src_word_emb.weight"].shape[0], (B, L))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    keys, spk = dev(state["encoder.src_word_emb.weight"][ids]), dev(state["speaker_emb.weight"][rng.integers(0, 4, B)])
    mel = dev((rng.standard_normal((B, T, M)) * 2 - 4).astype(np.float32))
    prior = dev(al.batch_prior(txt_lens, mel_lens, T, L))
    h = al.Aligner(M, M, H, 5e-4, device=0)
    blob = packer.pack_aligner(state)
    h.load_weights(blob)
    h.profile_enable(True)
    dur = torch.empty((B, L), device="cuda")
    attn = torch.empty((B, T, L), device="cuda")
    torch.cuda.synchronize()
    rows = {"proj": [], "attn": [], "mas": [], "call_wall": []}
    if a.prior == "host":
        rows["host_prior"] = []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        if a.prior == "host":
            prior = dev(al.batch_prior(txt_lens, mel_lens, T, L))
            torch.cuda.synchronize()
            built = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
        h.align(mel, keys, spk, txt_lens, mel_lens, "device" if a.prior == "device" else prior, out_dur=dur, want=())
        wall = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            ms = h.profile_read()
            for k in ("proj", "attn", "mas"):
                rows[k].append(ms[k])
            rows["call_wall"].append(wall)
            if a.prior == "host":
                rows["host_prior"].append(built)
    out = {f"{k}_ms": round(statistics.median(v), 4) for k, v in rows.items()}
    out.update(prior=a.prior, B=B, L=L, T=T, hidden=H, n_mel=M, repeats=a.repeats, device_bytes=h.device_bytes(), weight_bytes=int(blob.size),
               map_bytes=B * T * L * 4, reference_4d_tensor_bytes=B * M * T * L * 4)
    out["maps_held"] = round((out["device_bytes"] - out["weight_bytes"]) / out["map_bytes"], 3)
    if not a.no_cpu:
        h.align(mel, keys, spk, txt_lens, mel_lens, prior, out_dur=dur, out_attn=attn, want=())
        host, gpu_dur = attn.cpu().numpy(), dur.cpu().numpy()
        from multiprocessing import get_context
        t0 = time.perf_counter()
        with get_context("spawn").Pool(a.cpus) as pool:
            cpu_dur = pool.map(_cpu_mas, [(host[b], int(txt_lens[b]), int(mel_lens[b])) for b in range(B)])
        out["numpy_loop_mas_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["numpy_cpus"] = a.cpus
        out["rows_equal_numpy"] = int(sum(np.array_equal(cpu_dur[b], gpu_dur[b, :txt_lens[b]]) for b in range(B)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
