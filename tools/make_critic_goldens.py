#!/usr/bin/env python3
"""Generate tests/golden/critic_*.npz by running the REFERENCE's own discriminators and losses on the CPU, unmodified:
MultiPeriodDiscriminator / MultiScaleDiscriminator (e2e_tts/models/vocoder/discriminator.py, layers.py:72-133) in eval() and
feature_loss / discriminator_loss / generator_loss (loss.py), once in float32 and once as a .double() copy, through the stand-in ``numba``
of oracle/make_goldens.py.  Needs the reference checkout; runs on the development machine only.

Weights are e2e_tts_amd.synth_weights.synth_critic_state(seed) at the default widths: a fixture stores the seed and the state's hash, not
the tensors.  The input is a tone plus noise (y) and a detuned, re-noised copy (g).

Every fixture holds: seed, state_hash, y / g [B, n] float32, lens; per discriminator d and map l a strided sample of the map (every 997th
element of the reference's [B, C, T(, p)] tensor, every element of a small one) as idx_d_l and r32 / r64 / g32 / g64_d_l; the raw scores
s{r,g}{32,64}_d; per row the figures fig32 / fig64 (fm [D, L], d_real, d_fake, g_fake [D] and the six losses, see FIG_NAMES) computed by
the reference's loss functions on the row's slice; fig32d_fm [B, D, L] and fig32d_mom [B, D, 3], the float32 run's means evaluated in
float64 from its maps (what the bars are bounds of: torch's own float32 scalar adds the rounding of a float32 mean); batch32 / batch64, the same six losses on the whole batch; and the bars: bound_fm
[B, D, L] = mean |r32 - r64| + mean |g32 - g64| and bound_mom [B, D, 3] = mean (|derivative| |d32 - d64|) for d_real, d_fake, g_fake --
triangle-inequality bounds of the reference's own float32 error, from its maps, never from differences of scalar figures.
critic_n2049.npz also holds a strided sample of every layer's effective weight (w_d_l, widx_d_l) as the reference's modules computed it.

Usage:  python tools/make_critic_goldens.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from e2e_tts_amd import critic as crit, synth_weights as sw  # noqa: E402
from oracle.make_goldens import GOLD, import_reference  # noqa: E402

SEED = 2024
STRIDE = 997
FIG_NAMES = ("feature_loss_mpd", "feature_loss_msd", "disc_loss_mpd", "disc_loss_msd", "gen_loss_mpd", "gen_loss_msd")
MAX_L = 8   # maps per discriminator in the default tables (7 + post)


def state_hash(*states) -> str:
    h = hashlib.sha256()
    for sd in states:
        for k in sorted(sd):
            h.update(k.encode() + b"\0" + np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def signals(B, n, seed):
    r = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    y = np.stack([0.5 * np.sin(2 * np.pi * (220.0 + 30 * b) * t) + 0.05 * r.standard_normal(n) for b in range(B)])
    g = np.stack([0.45 * np.sin(2 * np.pi * (221.5 + 30 * b) * t + 0.1) + 0.05 * r.standard_normal(n) for b in range(B)])
    return y.astype(np.float32), g.astype(np.float32)


def sample_index(size):
    step = max(1, min(STRIDE, size // 64))
    return np.arange(0, size, step, dtype=np.int64)


def run(models, states, y, g, dtype):
    import torch
    from models.vocoder.discriminator import MultiPeriodDiscriminator, MultiScaleDiscriminator
    nets = []
    for cls, sd in zip((MultiPeriodDiscriminator, MultiScaleDiscriminator), states):
        m = cls()
        m.load_state_dict(sw.to_torch(sd))
        nets.append(m.eval().to(dtype))
    yt, gt = torch.from_numpy(y).to(dtype)[:, None, :], torch.from_numpy(g).to(dtype)[:, None, :]
    out = []
    with torch.no_grad():
        for m in nets:
            out.append(m(yt, gt))   # y_d_rs, y_d_gs, fmap_rs, fmap_gs
    return nets, out


def losses(fr, fg, sr, sg):
    """The reference's three functions on (a slice of) one family's outputs -> (feature, discriminator, generator) as floats, and the
    per-discriminator terms."""
    import torch
    from models.vocoder.loss import discriminator_loss, feature_loss, generator_loss
    fl = float(feature_loss(fr, fg))
    dl, r_l, g_l = discriminator_loss(sr, sg)
    gl, gen = generator_loss(sg)
    fm = [[float(torch.mean(torch.abs(a - b))) for a, b in zip(dr, dg)] for dr, dg in zip(fr, fg)]
    return fl, float(dl), float(gl), fm, r_l, g_l, [float(v) for v in gen]


def case(models, name, B, n, states, with_weights=False):
    import torch
    y, g = signals(B, n, seed=n + B)
    arrays = dict(seed=np.int64(SEED), state_hash=np.frombuffer(state_hash(*states).encode(), np.uint8), y=y, g=g, lens=np.full(B, n, np.int64))
    res = {}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        nets, out = run(models, states, y, g, dtype)
        res[tag] = out
        if with_weights and tag == "32":
            d = 0
            for net in nets:
                for disc in net.discriminators:
                    for l, conv in enumerate(list(disc.convs) + [disc.conv_post]):
                        w = conv.weight.detach().numpy().reshape(-1)
                        idx = sample_index(w.size)
                        arrays[f"widx_{d}_{l}"], arrays[f"w_{d}_{l}"] = idx, w[idx].astype(np.float32)
                    d += 1
    D = sum(len(o[0]) for o in res["32"])
    fig = {t: dict(fm=np.full((B, D, MAX_L), np.nan), d_real=np.zeros((B, D)), d_fake=np.zeros((B, D)), g_fake=np.zeros((B, D)), loss=np.zeros((B, 6)))
           for t in ("32", "64")}
    batch = {t: np.zeros(6) for t in ("32", "64")}
    bound_fm, bound_mom = np.full((B, D, MAX_L), np.nan), np.zeros((B, D, 3))
    fig32d_fm, fig32d_mom = np.full((B, D, MAX_L), np.nan), np.zeros((B, D, 3))
    d0 = 0
    for fam in range(2):
        for tag in ("32", "64"):
            sr, sg, fr, fg = res[tag][fam]
            fl, dl, gl, *_ = losses(fr, fg, sr, sg)
            batch[tag][fam], batch[tag][2 + fam], batch[tag][4 + fam] = fl, dl, gl
            for b in range(B):
                cut = lambda xs: [x[b:b + 1] for x in xs]  # noqa: E731
                fl, dl, gl, fm, r_l, g_l, gen = losses([cut(m) for m in fr], [cut(m) for m in fg], cut(sr), cut(sg))
                f = fig[tag]
                f["loss"][b, fam], f["loss"][b, 2 + fam], f["loss"][b, 4 + fam] = fl, dl, gl
                for i in range(len(sr)):
                    f["fm"][b, d0 + i, :len(fm[i])] = fm[i]
                    f["d_real"][b, d0 + i], f["d_fake"][b, d0 + i], f["g_fake"][b, d0 + i] = r_l[i], g_l[i], gen[i]
        sr32, sg32, fr32, fg32 = res["32"][fam]
        sr64, sg64, fr64, fg64 = res["64"][fam]
        for i in range(len(sr32)):
            d = d0 + i
            for l in range(len(fr32[i])):
                r32, r64, g32, g64 = (t[i][l].numpy() for t in (fr32, fr64, fg32, fg64))
                rms = float(np.sqrt(np.mean(r64 ** 2)))
                if l < len(fr32[i]) - 1:
                    assert 1e-3 <= rms <= 1e2, (name, d, l, rms)
                idx = sample_index(r32.size)
                arrays[f"idx_{d}_{l}"] = idx
                for nm, a in (("r32", r32), ("r64", r64), ("g32", g32), ("g64", g64)):
                    arrays[f"{nm}_{d}_{l}"] = a.reshape(-1)[idx]
                for b in range(B):
                    bound_fm[b, d, l] = np.mean(np.abs(r32[b].astype(np.float64) - r64[b])) + np.mean(np.abs(g32[b].astype(np.float64) - g64[b]))
                    fig32d_fm[b, d, l] = np.mean(np.abs(r32[b].astype(np.float64) - g32[b].astype(np.float64)))
            a32, a64, b32, b64 = sr32[i].numpy().astype(np.float64), sr64[i].numpy(), sg32[i].numpy().astype(np.float64), sg64[i].numpy()
            for nm, a in (("sr32", sr32[i]), ("sr64", sr64[i]), ("sg32", sg32[i]), ("sg64", sg64[i])):
                arrays[f"{nm}_{d}"] = a.numpy()
            for b in range(B):
                bound_mom[b, d, 0] = np.mean(2 * np.abs(1 - a64[b]) * np.abs(a32[b] - a64[b]))
                bound_mom[b, d, 1] = np.mean(2 * np.abs(b64[b]) * np.abs(b32[b] - b64[b]))
                bound_mom[b, d, 2] = np.mean(2 * np.abs(1 - b64[b]) * np.abs(b32[b] - b64[b]))
                fig32d_mom[b, d] = np.mean((1 - a32[b]) ** 2), np.mean(b32[b] ** 2), np.mean((1 - b32[b]) ** 2)
        d0 += len(sr32)
    for t in ("32", "64"):
        for k, v in fig[t].items():
            arrays[f"fig{t}_{k}"] = v
        arrays[f"batch{t}"] = batch[t]
    arrays["bound_fm"], arrays["bound_mom"] = bound_fm, bound_mom
    arrays["fig32d_fm"], arrays["fig32d_mom"] = fig32d_fm, fig32d_mom
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, feature loss {batch['64'][:2]}, fp32 - fp64 {batch['32'] - batch['64']}", flush=True)


def main():
    models = import_reference()
    states = sw.synth_critic_state(SEED, crit.default_config())
    case(models, "critic_n2049", 1, 2049, states, with_weights=True)
    case(models, "critic_n3001", 1, 3001, states)
    case(models, "critic_b3_n1501", 3, 1501, states)
    case(models, "critic_n29", 1, 29, states)   # a short length at which no figure is a difference of nearly equal scores
    case(models, "critic_n12", 1, 12, states)   # the smallest length the reference runs, and the header's minimum


if __name__ == "__main__":
    main()
