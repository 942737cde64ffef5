#!/usr/bin/env python3
"""Generate tests/golden/forced_*.npz by running the REFERENCE's own teacher-forced forward on CPU, unmodified:
UnsupervisedFastSpeech2.forward in eval() (e2e_tts/models/acoustic/unsupervised_fastspeech2/model.py:95-153 -- what generate_mel,
src/tools/tools_for_data.py:216-256, calls), i.e. VarianceAdaptor.forward with attn_prior given (layers.py:175-272), through the stand-in
``numba`` of oracle/make_goldens.py.  The recipe of tools/make_aligner_goldens.py: weights are e2e_tts_amd.synth_weights states stored as
SEEDS, the mel is that tool's smooth random signal, the prior is the reference's beta-binomial prior.

Every model fixture holds: variant, weight_seed, data_seed, ids [B, L], speakers [B], txt_lens, mel_lens, mel [B, T, n_mel] (tiny cases), the
frame-level targets handed to forward (f0 / uv or pitch, energy: [B, T]), attn_soft [B, T, L] and attn_logprob_err of the fp32 module, and
per step s in (0, 10 ** 9) -- the soft expansion and the length regulator -- under the prefix ``s0_`` / ``s1_``: dur, mel_lens, the targets
as RETURNED (p_f0 / p_uv or p_pitch, e_tgt; absent when None), pitch_idx, energy_idx, pitch_pred, energy_pred, log_d, dec_in (forward
pre-hook of the first decoder block), mel, mel_post, and ``<name>_err`` = mean |fp32 - float64| of every float array over valid rows, from
the same module in .double().  ``row_stride``: the float arrays dec_in / mel / mel_post hold rows 0, stride, 2 stride, ... only (the full
case; 1 otherwise).  p_control: the pitch control of the partial case (variance_adaptor.forward's own argument, bound with a wrapper: the
model's forward does not pass one).

Data seeds are searched so that (a) the MAS path survives the aligner tool's perturbation screen (noise of 16 x max |attn_logprob fp32 -
float64| on log(attn), 32 trials) and (b) every bucket decision taken from a target or a prediction lies >= 1e-3 (bucket units) from its
boundary (oracle.make_goldens.margins).  tests/forced_ref.py's restatement is checked against the module before anything is written.

forced_get_f0.npz: get_f0 of the reference's data loader (Hz -> normalised f0 with interpolated unvoiced stretches, uv) on six tracks, both
pitch quantizations; e2e_tts_amd.models.f0_targets restates it.

forced_frame2phoneme.npz: the reference's frame2phoneme (function.py:155-166) run directly on rows with zero durations before, between and
after, and with phonemes of more than 8 and more than 128 frames (numpy's pairwise summation paths).

Usage:  python tools/make_forced_goldens.py [--only NAME]
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from e2e_tts_amd import aligner as al_py, config as cfgmod, synth_weights as sw  # noqa: E402
from oracle.make_goldens import GOLD, import_reference, margins, pv_variant  # noqa: E402
from make_aligner_goldens import smooth_mel  # noqa: E402
import aligner_ref as ar  # noqa: E402
import forced_ref as fr  # noqa: E402

STEPS = (0, 10 ** 9)
TRIALS, FACTOR = 32, 16.0
STATS = cfgmod.DEFAULT_STATS


def variant_config(variant):
    cfg = cfgmod.default_config() if variant == "full" else cfgmod.tiny_config()
    if variant in ("frame", "nouv"):
        cfg = pv_variant(cfg, variant)
    return cfg


def smooth(rng, B, T, width=9):
    x = rng.standard_normal((B, T + width - 1))
    k = np.hanning(width)
    k /= k.sum()
    return np.stack([np.convolve(x[b], k, mode="valid") for b in range(B)])


def make_targets(rng, B, T, mel_lens, use_uv, energy_bins, pitch_bins):
    """Frame-level targets as the data loader hands them over: normalised f0 with a 0 / 1 unvoiced mark (runs), or one pitch value per
    frame inside the pitch bins; energies inside the energy bins; zero past an utterance's end (the collate function's padding)."""
    f0 = (2.5 * smooth(rng, B, T)).astype(np.float32)
    uv = (smooth(rng, B, T, 13) > 0.15).astype(np.float32)
    lo, hi = float(pitch_bins[0]), float(pitch_bins[-1])
    pitch = (lo + (hi - lo) * (0.5 + 0.9 * smooth(rng, B, T))).astype(np.float32)
    lo, hi = float(energy_bins[0]), float(energy_bins[-1])
    energy = (lo + (hi - lo) * (0.5 + 0.9 * smooth(rng, B, T))).astype(np.float32)
    for b, m in enumerate(mel_lens):
        for a in (f0, uv, pitch, energy):
            a[b, m:] = 0.0
    return ({"f0": f0, "uv": uv} if use_uv else pitch), energy


def run_forward(m, dtype, speakers, ids, mel, prior, p_t, e_t, txt_lens, mel_lens, step):
    """The reference's forward with hooks.  -> dict of numpy arrays."""
    import torch
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dtype)  # noqa: E731
    tr = {}
    hooks = [m.variance_adaptor.pitch_embedding.register_forward_hook(lambda mod, i, o: tr.__setitem__("pitch_idx", i[0].numpy().copy())),
             m.variance_adaptor.energy_embedding.register_forward_hook(lambda mod, i, o: tr.__setitem__("energy_idx", i[0].numpy().copy())),
             m.decoder.layer_stack[0].register_forward_pre_hook(lambda mod, i: tr.__setitem__("dec_in", i[0].numpy().copy()))]
    pt = {k: t(v) for k, v in p_t.items()} if isinstance(p_t, dict) else t(p_t)
    L, T = ids.shape[1], mel.shape[1]
    inputs = (torch.from_numpy(speakers), torch.from_numpy(ids), t(mel), t(prior), pt, t(e_t), torch.from_numpy(txt_lens), L,
              torch.from_numpy(mel_lens), T)
    (mel_o, post, log_d, p_pred, e_pred, _, _, out_lens, _, attn_out), (p_ret, e_ret) = m(inputs, step=step)
    for h in hooks:
        h.remove()
    n = lambda v: v.numpy().copy()  # noqa: E731
    tr.update(mel=n(mel_o), mel_post=n(post), log_d=n(log_d), pitch_pred=n(p_pred), energy_pred=n(e_pred), mel_lens=n(out_lens).astype(np.int64),
              attn_soft=n(attn_out[0][:, 0]), dur=n(attn_out[2]).astype(np.float32), attn_logprob=n(attn_out[3][:, 0]))
    if isinstance(p_ret, dict):
        tr.update(p_f0=n(p_ret["f0"]), p_uv=n(p_ret["uv"]))
    elif p_ret is not None:
        tr["p_pitch"] = n(p_ret)
    if e_ret is not None:
        tr["e_tgt"] = n(e_ret)
    return tr


def valid_err(a32, a64, rows):
    """mean |fp32 - float64| over rows < rows[b] (axis 1)."""
    tot, cnt = 0.0, 0
    for b, r in enumerate(rows):
        d = np.abs(a32[b, :r].astype(np.float64) - a64[b, :r])
        tot += float(d.sum())
        cnt += d.size
    return tot / max(cnt, 1)


def target_margin(tr, cfg, state, txt_lens, p_control):
    """margins() on what the embeddings were looked up from: the returned targets, or prediction * control where there was none."""
    ve = cfg["models"]["fastspeech2"]["variance"]["variance_embedding"]
    out = dict(log_d=np.zeros_like(tr["log_d"]))
    controls = [1.0, 1.0, 1.0]
    if "p_f0" in tr:
        out["pitch_pred"] = np.stack([tr["p_f0"], np.where(tr["p_uv"] > 0, 1.0, -1.0)], -1)
    elif "p_pitch" in tr:
        out["pitch_pred"] = tr["p_pitch"]
    else:
        out["pitch_pred"] = tr["pitch_pred"] * np.float32(p_control) if ve["use_uv"] else tr["pitch_pred"]
        controls[1] = p_control
    out["energy_pred"] = tr["e_tgt"] if "e_tgt" in tr else tr["energy_pred"]
    mg = margins(out, state["variance_adaptor.energy_bins"], STATS, tuple(controls), txt_lens, ve, state["variance_adaptor.pitch_bins"])
    return min(mg["uv"], mg["f0"], mg["energy"])


def one_case(models, name, variant, B, L, T, txt_lens, mel_lens, weight_seed=1234, data_seed=1, pitch=True, energy=True, p_control=1.0, row_stride=1,
             store_mel=True):
    import torch
    torch.set_grad_enabled(False)
    cfg = variant_config(variant)
    fs = cfg["models"]["fastspeech2"]
    n_mel = cfg["audio"]["mel"]["channels"]
    use_uv = fs["variance"]["variance_embedding"]["use_uv"]
    p_frame = fs["variance"]["variance_embedding"]["pitch_feature"] == "frame_level"
    e_frame = fs["variance"]["variance_embedding"]["energy_feature"] == "frame_level"
    state = sw.make_acoustic_state(cfg, STATS, 4, seed=weight_seed, mode="varied")
    m = models.UnsupervisedFastSpeech2(n_symbols=cfgmod.N_SYMBOLS, n_speakers=4, n_channels=n_mel, config=fs, stats=STATS)
    m.load_state_dict(sw.to_torch(state), strict=True)
    m.eval()
    if p_control != 1.0:   # variance_adaptor.forward's own p_control argument; the model's forward leaves it at its default
        for mod in (m,):
            orig = mod.variance_adaptor.forward
            mod.variance_adaptor.forward = lambda *a, _o=orig, **k: _o(*a, p_control=p_control, **k)
    m64 = copy.deepcopy(m).double()
    if p_control != 1.0:
        orig64 = type(m64.variance_adaptor).forward.__get__(m64.variance_adaptor)
        m64.variance_adaptor.forward = lambda *a, **k: orig64(*a, p_control=p_control, **k)
    txt_lens, mel_lens = np.asarray(txt_lens, np.int64), np.asarray(mel_lens, np.int64)
    assert fs["variance"]["duration_modelling"]["binarization_start_steps"] <= STEPS[1]
    first = data_seed
    while True:
        rng = np.random.Generator(np.random.PCG64(data_seed))
        ids = np.zeros((B, L), np.int64)
        for b in range(B):
            ids[b, :txt_lens[b]] = rng.integers(1, cfgmod.N_SYMBOLS + 1, txt_lens[b])
        speakers = rng.integers(0, 4, B).astype(np.int64)
        mel = smooth_mel(rng, B, T, n_mel, mel_lens)
        prior = al_py.batch_prior(txt_lens, mel_lens, T, L)
        p_t, e_t = make_targets(rng, B, T, mel_lens, use_uv, state["variance_adaptor.energy_bins"], state["variance_adaptor.pitch_bins"])
        if not pitch:
            p_t = None
        if not energy:
            e_t = None
        runs = {}
        for si, step in enumerate(STEPS):
            cp = lambda v: None if v is None else ({k: a.copy() for k, a in v.items()} if isinstance(v, dict) else v.copy())  # noqa: E731
            r32 = run_forward(m, torch.float32, speakers, ids, mel, prior, cp(p_t), cp(e_t), txt_lens, mel_lens, step)
            r64 = run_forward(m64, torch.float64, speakers, ids, mel, prior, cp(p_t), cp(e_t), txt_lens, mel_lens, step)
            runs[si] = (r32, r64)
        r32, r64 = runs[0]
        hard_dur = r32["dur"]
        ok = np.array_equal(hard_dur, runs[1][0]["dur"]) and np.array_equal(hard_dur, r64["dur"])
        # the aligner tool's perturbation screen on the MAS path
        err_l = float(max(np.abs(r32["attn_logprob"][b, :mel_lens[b], :].astype(np.float64) - r64["attn_logprob"][b, :mel_lens[b], :]).max() for b in range(B)))
        amp = FACTOR * err_l
        with np.errstate(divide="ignore"):
            loga = np.log(r32["attn_soft"])
        hard = ar.b_mas(r32["attn_soft"], txt_lens, mel_lens)
        ok = ok and np.array_equal(hard.sum(1), hard_dur)
        nrng = np.random.Generator(np.random.PCG64(9000 + data_seed))
        for _ in range(TRIALS if ok else 0):
            noisy = (loga + nrng.uniform(-amp, amp, loga.shape).astype(np.float32)).astype(np.float32)
            if not np.array_equal(ar.b_mas(noisy, txt_lens, mel_lens, log_map=True, search=ar.mas_rows), hard):
                ok = False
                break
        mg = min(target_margin(runs[si][0], cfg, state, txt_lens, p_control) for si in runs) if ok else 0.0
        if ok and mg >= 1e-3:
            break
        print(f"  [{name}] data seed {data_seed}: screen ok {ok}, margin {mg:.2e}: trying the next seed", flush=True)
        data_seed += 1
        assert data_seed < first + 200, "no seed found"
    # the restatement against the module, before anything is written
    from e2e_tts_amd.packer import variance_position_table
    orc = fr.ForcedOracle(state, cfg, STATS, var_pos_table=variance_position_table(4096, fs["encoder_hidden"]))
    arrays = dict(variant=np.array(variant), weight_seed=np.int64(weight_seed), data_seed=np.int64(data_seed), ids=ids, speakers=speakers, txt_lens=txt_lens,
                  mel_lens=mel_lens, attn_soft=r32["attn_soft"], attn_logprob_err=np.float64(err_l), p_control=np.float64(p_control),
                  row_stride=np.int64(row_stride), margin=np.float64(mg), screen=np.array([amp, TRIALS, first, data_seed], np.float64))
    if store_mel:
        arrays["mel"] = mel
    if isinstance(p_t, dict):
        arrays.update(f0=p_t["f0"], uv=p_t["uv"])
    elif p_t is not None:
        arrays["pitch"] = p_t
    if e_t is not None:
        arrays["energy"] = e_t
    for si, step in enumerate(STEPS):
        r32, r64 = runs[si]
        soft = si == 0
        out_lens = r32["mel_lens"]
        cp = lambda v: None if v is None else ({k: a.copy() for k, a in v.items()} if isinstance(v, dict) else v.copy())  # noqa: E731
        omel, opost, olens, (op, oe) = orc.forward(speakers, ids, txt_lens, mel_lens, r32["dur"], r32["attn_soft"], cp(p_t), cp(e_t), soft=soft,
                                                   p_control=p_control, max_mel_len=T)
        assert np.array_equal(olens, out_lens), (olens, out_lens)
        assert np.array_equal(orc.trace["pitch_idx"], r32["pitch_idx"]) and np.array_equal(orc.trace["energy_idx"], r32["energy_idx"]), name
        for k, v in (("p_f0", op["f0"] if isinstance(op, dict) else None), ("p_uv", op["uv"] if isinstance(op, dict) else None),
                     ("p_pitch", None if isinstance(op, dict) else op), ("e_tgt", oe)):
            assert (v is None) == (k not in r32), (name, k)
            if v is not None:
                assert np.array_equal(v, r32[k]), (name, k, float(np.abs(v - r32[k]).max()))
        e_rest = max(valid_err(orc.trace["dec_in"], r32["dec_in"].astype(np.float64), out_lens), valid_err(opost, r32["mel_post"].astype(np.float64), out_lens))
        assert e_rest <= 1e-5, (name, e_rest)
        pre = f"s{si}_"
        n_p = out_lens if p_frame else txt_lens
        n_e = out_lens if e_frame else txt_lens
        rows_of = dict(dec_in=out_lens, mel=out_lens, mel_post=out_lens, log_d=txt_lens, pitch_pred=n_p, energy_pred=n_e, p_f0=n_p, p_pitch=n_p, e_tgt=n_e)
        arrays[pre + "dur"] = r32["dur"]
        arrays[pre + "mel_lens"] = out_lens
        arrays[pre + "pitch_idx"] = r32["pitch_idx"].astype(np.int32)
        arrays[pre + "energy_idx"] = r32["energy_idx"].astype(np.int32)
        if "p_uv" in r32:
            arrays[pre + "p_uv"] = r32["p_uv"]
        errs = []
        for k, rows in rows_of.items():
            if k not in r32:
                continue
            arrays[pre + k + "_err"] = np.float64(valid_err(r32[k], r64[k], rows))
            errs.append(f"{k} {float(arrays[pre + k + '_err']):.1e}")
            arrays[pre + k] = r32[k][:, ::row_stride] if k in ("dec_in", "mel", "mel_post") else r32[k]
        print(f"  [{name}] step {step}: T {r32['mel'].shape[1]} mel_lens {out_lens.tolist()}; restatement vs module {e_rest:.1e}; fp32 vs float64: " + ", ".join(errs),
              flush=True)
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"[{name}] seed {data_seed} margin {mg:.2e} -> {os.path.getsize(path) / 1024:.0f} KiB", flush=True)
    assert os.path.getsize(path) < 800 * 1024


def case_frame2phoneme(models):
    """The reference's own function on durations with zeros before, between and after, and on long phonemes."""
    from models.acoustic.unsupervised_fastspeech2.function import frame2phoneme
    rng = np.random.Generator(np.random.PCG64(5))
    rows = [[0, 0, 3, 1, 0, 2, 0, 0, 5, 1, 0], [2, 0, 0, 0, 4, 1, 1, 0], [0, 1], [1, 9, 17, 0, 137, 2, 300, 0, 0, 3, 8, 129], [3, 3, 3], [0, 0, 0, 0, 6, 0, 1]]
    T = 520
    L = max(len(r) for r in rows)
    dur = np.zeros((len(rows), L), np.float32)
    lens = np.array([len(r) for r in rows], np.int64)
    frames = rng.standard_normal((len(rows), T)).astype(np.float32)
    uv = (smooth(rng, len(rows), T, 13) > -0.2).astype(np.float32)
    out = np.zeros((len(rows), L), np.float32)
    out_uv = np.zeros((len(rows), L), np.float32)
    for b, r in enumerate(rows):
        dur[b, :len(r)] = r
        out[b, :len(r)] = frame2phoneme(np.asarray(r, np.int32), frames[b].copy())
        out_uv[b, :len(r)] = frame2phoneme(np.asarray(r, np.int32), uv[b].copy())
        assert np.array_equal(out[b, :len(r)], fr.frame2phoneme(np.asarray(r, np.int32), frames[b].copy()))
    assert np.array_equal(out, fr.get_phoneme_level(frames, lens, dur, L))
    path = os.path.join(GOLD, "forced_frame2phoneme.npz")
    np.savez_compressed(path, dur=dur, lens=lens, frames=frames, uv=uv, means=out, uv_means=out_uv)
    print(f"[forced_frame2phoneme] -> {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def case_get_f0():
    """get_f0 of the reference's data loader (src/tools/dataloader.py:185-196), the method's own text extracted with ``ast`` (the module's
    imports need packages this image lacks) and run on f0 tracks in Hz: voiced / unvoiced mixes, unvoiced ends, all unvoiced, all voiced."""
    import ast
    import tempfile
    import types
    from oracle.make_goldens import REF
    src = open(os.path.join(REF, "e2e_tts", "src", "tools", "dataloader.py")).read()
    fn = next(n for c in ast.parse(src).body if isinstance(c, ast.ClassDef) for n in c.body if isinstance(n, ast.FunctionDef) and n.name == "get_f0")
    import torch
    ns = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "dataloader.py", "exec"), ns)
    rng = np.random.Generator(np.random.PCG64(3))
    T = 40
    tracks = []
    for kind in range(6):
        hz = 120.0 + 60.0 * smooth(rng, 1, T)[0]
        uv = smooth(rng, 1, T, 7)[0] > 0.1
        if kind == 1:
            uv[:5] = True
            uv[-4:] = True
        if kind == 2:
            uv[:] = True
        if kind == 3:
            uv[:] = False
        hz[uv] = 0.0
        tracks.append(hz if kind != 4 else hz.astype(np.float32))
    arrays = {}
    tmp = tempfile.mkdtemp()
    for q in ("linear", "log"):
        for i, hz in enumerate(tracks):
            path = os.path.join(tmp, f"{i}.npy")
            np.save(path, hz)
            me = types.SimpleNamespace(prosody_path={"x": {"f0": path}}, pitch_eps=0.000000001, variance_config={"pitch_quantization": q}, stats=STATS)
            f0, uv = ns["get_f0"](me, "x")
            arrays[f"{q}_{i}_f0"], arrays[f"{q}_{i}_uv"] = f0.numpy(), uv.numpy()
            arrays[f"hz_{i}"] = hz
    path = os.path.join(GOLD, "forced_get_f0.npz")
    np.savez_compressed(path, n=np.int64(len(tracks)), **arrays)
    print(f"[forced_get_f0] -> {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    args = ap.parse_args()
    models = import_reference()
    jobs = {
        "forced_frame2phoneme": lambda: case_frame2phoneme(models),
        "forced_get_f0": case_get_f0,
        # T = 70 > tiny max_seq_len 60: the regenerated position table; a one-phoneme utterance
        "forced_tiny_b3": lambda: one_case(models, "forced_tiny_b3", "tiny", 3, 12, 70, (12, 7, 1), (70, 33, 5)),
        "forced_tiny_wide_b1": lambda: one_case(models, "forced_tiny_wide_b1", "tiny", 1, 70, 150, (70,), (150,), data_seed=20),
        "forced_tiny_frame_b3": lambda: one_case(models, "forced_tiny_frame_b3", "frame", 3, 12, 70, (12, 7, 1), (70, 33, 5), data_seed=40),
        "forced_tiny_nouv_b3": lambda: one_case(models, "forced_tiny_nouv_b3", "nouv", 3, 12, 70, (12, 7, 1), (70, 33, 5), data_seed=60),
        "forced_tiny_partial_b3": lambda: one_case(models, "forced_tiny_partial_b3", "tiny", 3, 12, 70, (12, 7, 1), (70, 33, 5), data_seed=80, pitch=False,
                                                   p_control=1.25),
        "forced_full_b2": lambda: one_case(models, "forced_full_b2", "full", 2, 40, 300, (40, 23), (300, 181), data_seed=100, row_stride=6, store_mel=False),
    }
    for name, fn in jobs.items():
        if args.only and name != args.only:
            continue
        fn()


if __name__ == "__main__":
    main()
