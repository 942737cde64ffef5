#!/usr/bin/env python3
"""Generate tests/golden/mel_*.npz by running the REFERENCE's own TorchSTFT.mel_spectrogram on CPU, unmodified: the class TorchSTFT
(e2e_tts/src/tools/stft.py:11-89) and dynamic_range_compression (src/tools/utils.py:22-28) are taken from their files with ``ast`` and
executed as they are, because the modules import librosa, which is not installed here (oracle/make_goldens.py: case_istft does the same for
inverse_stft).  ``librosa.filters.mel`` is stood in by e2e_tts_amd.mel.mel_filterbank -- or by a given dense matrix -- and the basis that
was used is stored in every fixture, so the fixtures pin the transform and not the filterbank formula.

The module is run in fp32 and, a deep copy of it, in .double() (its window, a plain attribute, is rebuilt in float64).  EVERY ROW IS RUN
ALONE AT ITS OWN LENGTH, since that is what the library computes (the reference, given one zero-padded batch, would reflect at the batch's
end).

Signals: a sine plus noise on the int16 grid, with a stretch of exact zeros and a stretch scaled by 1e-3 (the near-silent case) where the
row is long enough.  A fixture holds: n_fft, hop, win_length, n_mel, sr, fmin, fmax, clip, mel_basis [n_mel, bins], pcm [B, n] int16 (the
fp32 input is pcm / 32768, exact), n_valid, mel_lens, mel32 / mel64 [B, T, n_mel] CHANNELS-LAST and energy32 / energy64 [B, T] (zeros past
mel_lens), ref_err_mel / ref_err_energy = (mean, max) of |fp32 - float64| over the valid region, zero_frames [k, 3] = (row, first, last + 1)
of the frames that lie wholly inside the zero stretch.

mel_align_tiny_b3: wav -> the reference's mel -> the reference's AlignmentEncoder + b_mas durations with the tiny aligner weights the aligner
fixtures use (tools/make_aligner_goldens.py).  Robustness screen, run here on the CPU: the fp32 mel is perturbed by uniform noise of 10 x
the derived per-element mel bar (tests/mel_ref.py), SCREEN_TRIALS times; a row is kept (screened = 1) only if its durations never change;
the data seed is advanced until every row is kept.  screen = [factor, trials, data seed tried first, data seed kept].

Usage:  python tools/make_mel_goldens.py
"""
from __future__ import annotations

import ast
import copy
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from e2e_tts_amd import mel as mel_py, synth_weights as sw  # noqa: E402
from oracle.make_goldens import GOLD, REF, import_reference  # noqa: E402
import mel_ref as mr  # noqa: E402

SCREEN_FACTOR, SCREEN_TRIALS = 10.0, 16


def reference_classes(basis_fn):
    """(TorchSTFT, dynamic_range_compression) of the reference, with ``librosa.filters.mel`` stood in by ``basis_fn(sr=, n_fft=, ...)``."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    src = open(os.path.join(REF, "e2e_tts", "src", "tools", "utils.py")).read()
    drc = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "dynamic_range_compression"]
    src = open(os.path.join(REF, "e2e_tts", "src", "tools", "stft.py")).read()
    cls = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "TorchSTFT"]
    librosa = types.SimpleNamespace(filters=types.SimpleNamespace(mel=basis_fn))
    ns = {"torch": torch, "nn": nn, "F": F, "librosa": librosa}
    exec(compile(ast.Module(body=drc + cls, type_ignores=[]), "reference:stft.py:TorchSTFT", "exec"), ns)
    return ns["TorchSTFT"], ns["dynamic_range_compression"]


def signal(rng, n, sr, zero=None, quiet=None):
    t = np.arange(n) / sr
    f0 = sr * rng.uniform(0.02, 0.08)
    x = 0.45 * np.sin(2 * np.pi * f0 * t + rng.uniform(0, 6.28)) + 0.2 * np.sin(2 * np.pi * 2.7 * f0 * t) + 0.08 * rng.standard_normal(n)
    if quiet:
        x[quiet[0]:quiet[1]] *= 1e-3
    if zero:
        x[zero[0]:zero[1]] = 0.0
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def run_rows(mods, pcm, n_valid, hop):
    """The fp32 and the float64 module on every row alone -> mel32, energy32, mel64, energy64 (channels-last, zeros past mel_lens)."""
    import torch
    m32, m64 = mods
    lens = np.asarray(n_valid) // hop
    B, T, M = len(n_valid), int(lens.max()), m32.n_mel_channels
    out = [np.zeros((B, T, M), np.float32), np.zeros((B, T), np.float32), np.zeros((B, T, M), np.float64), np.zeros((B, T), np.float64)]
    for b in range(B):
        x = torch.from_numpy(pcm[b, :n_valid[b]].astype(np.float32) / np.float32(32768.0))[None]
        for k, (mod, xx) in enumerate(((m32, x), (m64, x.double()))):
            mel, energy = mod.mel_spectrogram(xx, return_energy=True)
            assert mel.shape == (1, M, lens[b]) and energy.shape == (1, lens[b]), (mel.shape, energy.shape)
            out[2 * k][b, :lens[b]] = mel[0].T.numpy()
            out[2 * k + 1][b, :lens[b]] = energy[0].numpy()
    return out


def make_modules(n_fft, hop, win, n_mel, sr, fmin, fmax, basis):
    import torch
    TorchSTFT, _ = reference_classes(lambda sr, n_fft, n_mels, fmin, fmax: basis)
    m32 = TorchSTFT(n_fft, hop, win, n_mel, sr, fmin, fmax)
    m64 = copy.deepcopy(m32).double()
    m64.window = torch.hann_window(win, dtype=torch.float64)
    assert m64.mel_basis.dtype == torch.float64 and np.array_equal(m32.mel_basis.numpy(), basis)
    return m32, m64


def one_case(name, n_fft, hop, n_mel, sr, fmin, fmax, frames_extra, seed, basis=None, zero_quiet=True):
    torch = __import__("torch")
    torch.set_grad_enabled(False)
    rng = np.random.Generator(np.random.PCG64(seed))
    win = n_fft
    if basis is None:
        basis = mel_py.mel_filterbank(sr, n_fft, n_mel, fmin, fmax)
    mods = make_modules(n_fft, hop, win, n_mel, sr, fmin, fmax, basis)
    n_valid = np.array([f * hop + e for f, e in frames_extra], np.int64)
    B, n = len(n_valid), int(n_valid.max())
    pcm = np.zeros((B, n), np.int16)
    zero_frames = []
    half = (n_fft - hop) // 2
    for b, nv in enumerate(n_valid):
        zero = quiet = None
        if zero_quiet and nv >= 5 * n_fft:
            z0 = int(nv * 0.3)
            zero = (z0, z0 + n_fft + 2 * hop)
            q0 = int(nv * 0.65)
            quiet = (q0, q0 + n_fft + 2 * hop)
            # frame f covers samples f * hop - half .. f * hop - half + n_fft - 1 of the row
            f0 = -(-(zero[0] + half) // hop)
            f1 = (zero[1] - n_fft + half) // hop + 1
            zero_frames.append((b, f0, f1))
        pcm[b, :nv] = signal(rng, int(nv), sr, zero, quiet)
    mel32, e32, mel64, e64 = run_rows(mods, pcm, n_valid, hop)
    lens = n_valid // hop
    for b, f0, f1 in zero_frames:
        assert f1 > f0 and (mel64[b, f0:f1] == np.log(1e-5)).all(), (name, b, f0, f1)
    # the restatement against the reference, before anything is written
    audio = pcm.astype(np.float32) / np.float32(32768.0)
    r64 = mr.mel_batch(audio.astype(np.float64), n_valid, mr.dft64(n_fft, win), basis.astype(np.float64), hop, dtype=np.float64)
    d64 = max(mr.valid_stats(r64[0], mel64, lens)[1], mr.valid_stats(r64[1], e64, lens)[1] / max(1.0, float(e64.max())))
    assert d64 <= 1e-9, (name, d64)
    err_m, err_e = mr.valid_stats(mel32, mel64, lens), mr.valid_stats(e32, e64, lens)
    arrays = dict(n_fft=np.int64(n_fft), hop=np.int64(hop), win_length=np.int64(win), n_mel=np.int64(n_mel), sr=np.int64(sr), fmin=np.float64(fmin),
                  fmax=np.float64(fmax), clip=np.float64(1e-5), mel_basis=basis.astype(np.float32), pcm=pcm, n_valid=n_valid, mel_lens=lens,
                  mel32=mel32, energy32=e32, mel64=mel64, energy64=e64, ref_err_mel=np.array(err_m), ref_err_energy=np.array(err_e),
                  zero_frames=np.array(zero_frames, np.int64).reshape(-1, 3))
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"  [{name}] frames {lens.tolist()}: reference fp32 vs float64 mel mean {err_m[0]:.3e} max {err_m[1]:.3e}; energy mean {err_e[0]:.3e} max "
          f"{err_e[1]:.3e}; restatement float64 vs reference float64 {d64:.1e}; zero frames {zero_frames}; {os.path.getsize(path) / 1024:.0f} KiB", flush=True)
    assert os.path.getsize(path) < 400 * 1024
    return arrays


def align_case(name="mel_align_tiny_b3", data_seed=1):
    import importlib
    import torch
    import make_aligner_goldens as mag
    from e2e_tts_amd import config as cfgmod
    import aligner_ref as ar
    torch.set_grad_enabled(False)
    import_reference()
    layers = importlib.import_module("models.acoustic.unsupervised_fastspeech2.layers")
    function = importlib.import_module("models.acoustic.unsupervised_fastspeech2.function")
    ref_prior = mag.reference_prior_function()
    tiny = cfgmod.tiny_config()
    H, M = tiny["models"]["fastspeech2"]["encoder_hidden"], tiny["audio"]["mel"]["channels"]
    n_fft, hop, sr, fmin, fmax, temperature, weight_seed = 1024, 256, 22050, 0.0, 8000.0, 5e-4, 77
    basis = mel_py.mel_filterbank(sr, n_fft, M, fmin, fmax)
    mods = make_modules(n_fft, hop, n_fft, M, sr, fmin, fmax, basis)
    state = sw.make_aligner_state(H, M, seed=weight_seed, weight_scale=1.0)
    enc = layers.AlignmentEncoder(M, M, H, temperature)
    enc.load_state_dict(sw.to_torch({k[len(mag.PREFIX):]: v for k, v in state.items() if k.startswith(mag.PREFIX)}), strict=True)
    enc.eval()
    txt_lens = np.array([7, 5, 2], np.int64)
    n_valid = np.array([26 * hop + 100, 17 * hop, 6 * hop + 31], np.int64)
    B, L, n = 3, int(txt_lens.max()), int(n_valid.max())
    lens = n_valid // hop
    T = int(lens.max())

    def durations(mel):
        priors = [torch.from_numpy(ref_prior(int(p), int(m), 1.0)) for p, m in zip(txt_lens, lens)]
        prior = torch.zeros(B, T, L)
        for b in range(B):
            prior[b, :priors[b].size(0), :priors[b].size(1)] = priors[b]
        a32, _ = mag.run_module(enc, mel, keys, txt_lens, prior.numpy(), spk, torch.float32)
        hard = function.b_mas(a32[:, None], txt_lens, lens, width=1)[:, 0]
        return hard.sum(1).astype(np.float32), prior.numpy().copy()

    first = data_seed
    while True:
        rng = np.random.Generator(np.random.PCG64(data_seed))
        ids = np.zeros((B, L), np.int64)
        for b in range(B):
            ids[b, :txt_lens[b]] = rng.integers(1, cfgmod.N_SYMBOLS + 1, txt_lens[b])
        speakers = rng.integers(0, 4, B).astype(np.int64)
        keys = state["encoder.src_word_emb.weight"][ids]
        spk = state["speaker_emb.weight"][speakers]
        pcm = np.zeros((B, n), np.int16)
        for b, nv in enumerate(n_valid):
            pcm[b, :nv] = signal(rng, int(nv), sr)
        mel32, e32, mel64, e64 = run_rows(mods, pcm, n_valid, hop)
        dur, prior = durations(mel32)
        g = dict(n_fft=n_fft, hop=hop, win_length=n_fft, clip=1e-5, mel_basis=basis)
        bar_mel, _ = mr.derived_bars(pcm.astype(np.float32) / np.float32(32768.0), n_valid, g)
        nrng = np.random.Generator(np.random.PCG64(9000 + data_seed))
        keep = np.ones(B, bool)
        for _ in range(SCREEN_TRIALS):
            noisy = (mel32 + SCREEN_FACTOR * bar_mel * nrng.uniform(-1, 1, mel32.shape)).astype(np.float32)
            d2, _ = durations(noisy)
            keep &= (d2 == dur).all(1)
        print(f"  [{name}] data seed {data_seed}: rows kept by the screen {keep.tolist()}; largest perturbation {SCREEN_FACTOR * bar_mel.max():.3e}", flush=True)
        if keep.all():
            break
        data_seed += 1
        assert data_seed < first + 30, "no robust seed found"
    assert all(dur[b, :txt_lens[b]].sum() == lens[b] for b in range(B))
    arrays = dict(n_fft=np.int64(n_fft), hop=np.int64(hop), win_length=np.int64(n_fft), n_mel=np.int64(M), sr=np.int64(sr), fmin=np.float64(fmin),
                  fmax=np.float64(fmax), clip=np.float64(1e-5), mel_basis=basis, pcm=pcm, n_valid=n_valid, mel_lens=lens, mel32=mel32, energy32=e32,
                  mel64=mel64, energy64=e64, ref_err_mel=np.array(mr.valid_stats(mel32, mel64, lens)), ref_err_energy=np.array(mr.valid_stats(e32, e64, lens)),
                  zero_frames=np.zeros((0, 3), np.int64), hidden=np.int64(H), temperature=np.float64(temperature), weight_seed=np.int64(weight_seed),
                  weight_scale=np.float64(1.0), ids=ids, speakers=speakers, txt_lens=txt_lens, dur=dur, screened=keep.astype(np.int64),
                  screen=np.array([SCREEN_FACTOR, SCREEN_TRIALS, first, data_seed], np.float64))
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"  [{name}] frames {lens.tolist()} txt_lens {txt_lens.tolist()} durations {[dur[b, :txt_lens[b]].astype(int).tolist() for b in range(B)]}; "
          f"{os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def main():
    os.makedirs(GOLD, exist_ok=True)
    # the top bins (above fmax = 1500 Hz of 2000) have zero weight in every filter; rows of 37 (+5 samples), 32 and 2 (+6 samples) frames
    one_case("mel_tiny_b3", 128, 32, 12, 4000, 0.0, 1500.0, ((37, 5), (32, 0), (2, 6)), seed=11)
    rng = np.random.Generator(np.random.PCG64(5))
    dense = (rng.random((12, 33)) * 0.01).astype(np.float32)   # a dense non-negative basis: every row's band is all 33 bins
    one_case("mel_tiny_dense_b2", 64, 32, 12, 4000, 0.0, 2000.0, ((21, 3), (9, 0)), seed=12, basis=dense)
    one_case("mel_full_b2", 1024, 256, 80, 22050, 0.0, 8000.0, ((40, 0), (33, 77)), seed=13)
    one_case("mel_48k_b1", 2048, 512, 80, 48000, 0.0, 24000.0, ((20, 0),), seed=14)
    align_case()


if __name__ == "__main__":
    main()
