#!/usr/bin/env python3
"""Generate tests/golden/denoiser.npz by running the REFERENCE's own vocoder-bias denoiser on CPU
(e2e_tts/models/vocoder/denoiser.py: STFT :55-153, Denoiser :156-186), unmodified.

The module cannot be imported or constructed as it stands in this image; three stand-ins, in this process only, make it run:
  * ``librosa.util`` (absent): ``normalize(x, norm=None)`` is the identity, ``pad_center`` centre-pads with zeros (the identity when the
    window already has filter_length points), ``tiny(x)`` is ``np.finfo(x.dtype).tiny`` -- the same kind of stand-in as the ``numba`` one of
    oracle/make_goldens.py;
  * ``torch.Tensor.cuda`` / ``nn.Module.cuda`` return self (the module is wired to ``.cuda()``);
  * the constructor's ``melgan`` is any object with an ``.inference`` (the reference's HifiGan has none): here the vocoder's forward, or a
    synthetic hum generator.
For the float64 yardstick the module is cast with ``.double()``; its forward casts the audio with ``.float()``, which is made the identity
for that run alone.

Stored (every row is run through the reference ALONE, trimmed to its length: what the engine's per-row reflection must equal):
  a_*   geometry (1024, 4): audio [3, 4096] with 4096 / 2816 / 768 valid samples (768 is the shortest legal length: both reflections fall
        into the same frames), strengths 0.1 and 0, the bias used, the fp32 output, the output of the module in .double(), their distances
        (mean-L1 ``dref``, max-abs ``dmax``) and the size of the effect (mean-L1 of output - input);
  b_*   the same for geometry (512, 2) on 2 x 2048 samples: at 2-fold overlap the Hann^2 envelope is not constant;
  c_*   calibration: the tiny-config HiFi-GAN with this project's synthetic weights (voc_micro_tiny's recipe), ``Denoiser(vocoder)``'s bias
        spectrum and bias audio for the zero mel, and the audio that vocoder makes of voc_micro_tiny's mel with its denoised output;
  d_*   every 37th row of both bases of geometry (1024, 4) and their L1 norms.
Before anything is written the tool checks that tests/denoiser_ref.py in float64 is the reference's float64 run (<= 1e-12) and that each
effect is at least 100 x dref.

Usage:  python tools/make_denoiser_goldens.py
"""
from __future__ import annotations

import copy
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from e2e_tts_amd import config as cfgmod, synth_weights as sw  # noqa: E402
from e2e_tts_amd.denoiser import centre_pad, stft_bases  # noqa: E402
from oracle.make_goldens import GOLD, import_reference  # noqa: E402
import denoiser_ref as dr  # noqa: E402


def install_standins():
    import torch
    util = types.ModuleType("librosa.util")
    util.normalize = lambda x, norm=None: x
    util.pad_center = lambda data, size: centre_pad(np.asarray(data), size)
    util.tiny = lambda x: np.finfo(np.asarray(x).dtype).tiny
    lib = types.ModuleType("librosa")
    lib.util = util
    sys.modules["librosa"], sys.modules["librosa.util"] = lib, util
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self


class Hum:
    """A stand-in vocoder for (a) and (b): whatever the mel, a fixed hum with some hiss, [1, 1, T * 256]."""

    def __init__(self, seed):
        self.seed = seed

    def inference(self, mel):
        import torch
        n = mel.shape[-1] * 256
        rng = np.random.Generator(np.random.PCG64(self.seed))
        t = np.arange(n) / 22050.0
        x = 0.02 * np.sin(2 * np.pi * 100.0 * t) + 0.01 * np.sin(2 * np.pi * 300.0 * t + 0.7) + 0.02 * rng.standard_normal(n)
        return torch.from_numpy(x.astype(np.float32))[None, None, :]


def speech_like(rng, B, n, amp=0.3):
    t = np.arange(n) / 22050.0
    x = np.zeros((B, n))
    for b in range(B):
        for h in range(1, 9):
            x[b] += rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * (110.0 + 23.0 * b) * h * t * (1.0 + 0.02 * np.sin(2 * np.pi * 3.0 * t)) + rng.uniform(0, 6.28))
        x[b] *= 0.6 + 0.4 * np.sin(2 * np.pi * 4.0 * t + b)
    x = amp * x / np.abs(x).max() + 0.02 * rng.standard_normal((B, n))
    return x.astype(np.float32)


def run_rows(den, audio, n_valid, strength, double=False):
    """Each row through the reference alone, trimmed to its length; zeros past it."""
    import torch
    out = np.zeros(audio.shape, np.float64 if double else np.float32)
    keep = torch.Tensor.float
    if double:
        den = copy.deepcopy(den).double()
        torch.Tensor.float = lambda self: self
    try:
        for b, nb in enumerate(n_valid):
            x = torch.from_numpy(audio[b:b + 1, :nb].astype(np.float64 if double else np.float32))
            out[b, :nb] = den(x, strength=strength)[0, 0].numpy()
    finally:
        torch.Tensor.float = keep
    return out


def valid_stats(a, b, n_valid):
    d = np.concatenate([np.abs(a[i, :nb].astype(np.float64) - b[i, :nb].astype(np.float64)) for i, nb in enumerate(n_valid)])
    return float(d.mean()), float(d.max())


def geometry_case(dmod, tag, N, V, audio, n_valid, strengths, arrays):
    import torch
    hop = N // V
    den = dmod.Denoiser(Hum(11), filter_length=N, n_overlap=V, win_length=N)
    bias = den.bias_spec[0, :, 0].numpy().copy()
    fwd, inv, win_sq = stft_bases(N, hop, N)
    np.testing.assert_array_equal(fwd, den.stft.forward_basis[:, 0, :].numpy())    # stft_bases is the reference's construction
    np.testing.assert_array_equal(inv, den.stft.inverse_basis[:, 0, :].numpy())
    arrays.update({f"{tag}_geometry": np.array([N, V], np.int64), f"{tag}_audio": audio, f"{tag}_n_valid": np.asarray(n_valid, np.int64),
                   f"{tag}_bias": bias, f"{tag}_strengths": np.asarray(strengths, np.float64)})
    dref, dmax, eff = [], [], []
    for i, s in enumerate(strengths):
        o32, o64 = run_rows(den, audio, n_valid, s), run_rows(den, audio, n_valid, s, double=True)
        r64 = dr.denoise_batch(dr.denoise_frames, audio, n_valid, bias, s, fwd, inv, win_sq, hop, dtype=np.float64)
        r32 = dr.denoise_batch(dr.denoise_rows, audio, n_valid, bias, s, fwd, inv, win_sq, hop)
        e64 = valid_stats(r64, o64, n_valid)[1]
        m, x = valid_stats(o32, o64, n_valid)
        ef = valid_stats(o32, audio, n_valid)[0]
        print(f"  [{tag}] strength {s}: reference fp32 vs float64 mean {m:.3e} max {x:.3e}; effect {ef:.3e}; restatement float64 vs reference "
              f"float64 max {e64:.2e}; 4-tap float32 vs reference float64 mean {valid_stats(r32, o64, n_valid)[0]:.3e}", flush=True)
        assert e64 <= 1e-12, e64
        if s > 0:
            assert ef >= 100 * m, (ef, m)
        arrays[f"{tag}_out32_s{i}"], arrays[f"{tag}_out64_s{i}"] = o32, o64
        dref.append(m), dmax.append(x), eff.append(ef)
    arrays[f"{tag}_dref"], arrays[f"{tag}_dmax"], arrays[f"{tag}_effect"] = np.array(dref), np.array(dmax), np.array(eff)
    torch.set_grad_enabled(False)


def calibration_case(models, dmod, arrays, strength=0.1):
    import torch
    config = cfgmod.tiny_config()
    voc_state = sw.make_vocoder_state(config, seed=4321)
    v = models.HifiGan(config["models"]["hifigan"])
    v.load_state_dict(sw.to_torch(voc_state), strict=True)
    v.eval()
    torch.set_grad_enabled(False)
    holder = types.SimpleNamespace(inference=v.forward)
    den = dmod.Denoiser(holder)                                   # (1024, 4), mode='zeros': 88 zero frames
    bias = den.bias_spec[0, :, 0].numpy().copy()
    bias_audio = v(torch.zeros((1, 80, 88)))[0, 0].numpy().copy()
    mel = np.load(os.path.join(GOLD, "voc_micro_tiny.npz"))["mel"]
    audio = v(torch.from_numpy(mel))[:, 0].numpy().copy()
    nv = [audio.shape[1]] * audio.shape[0]
    o32, o64 = run_rows(den, audio, nv, strength), run_rows(den, audio, nv, strength, double=True)
    m, x = valid_stats(o32, o64, nv)
    ef = valid_stats(o32, audio, nv)[0]
    print(f"  [c] bias L1 {np.abs(bias).sum():.4e} (max {bias.max():.3e}); audio {audio.shape} mean|x| {np.abs(audio).mean():.3e}; strength {strength}: "
          f"reference fp32 vs float64 mean {m:.3e} max {x:.3e}; effect {ef:.3e}", flush=True)
    assert ef >= 100 * m, (ef, m)
    arrays.update(c_bias_spec=bias, c_bias_audio=bias_audio, c_mel=mel, c_audio=audio, c_out32=o32, c_out64=o64, c_strength=np.float64(strength),
                  c_dref=np.float64(m), c_dmax=np.float64(x), c_effect=np.float64(ef), c_weight_seed=np.int64(4321))


def main():
    models = import_reference()
    install_standins()
    dmod = importlib.import_module("models.vocoder.denoiser")
    arrays = {}
    rng = np.random.Generator(np.random.PCG64(2024))
    geometry_case(dmod, "a", 1024, 4, speech_like(rng, 3, 4096), [4096, 2816, 768], (0.1, 0.0), arrays)
    geometry_case(dmod, "b", 512, 2, speech_like(rng, 2, 2048), [2048, 2048], (0.1, 0.0), arrays)
    calibration_case(models, dmod, arrays)
    fwd, inv, _ = stft_bases(1024, 256, 1024)
    rows = np.arange(0, fwd.shape[0], 37)
    arrays.update(d_rows=rows, d_fwd_rows=fwd[rows], d_inv_rows=inv[rows], d_fwd_l1=np.float64(np.abs(fwd.astype(np.float64)).sum()),
                  d_inv_l1=np.float64(np.abs(inv.astype(np.float64)).sum()))
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "denoiser.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  wrote {path} ({size / 1024:.0f} KiB)", flush=True)
    assert size < 900 * 1024, f"{path} is {size} bytes: committed files stay well under 1 MiB"


if __name__ == "__main__":
    main()
