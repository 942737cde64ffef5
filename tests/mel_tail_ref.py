"""mel_tail_kernel (csrc/mel/mel.hip) restated alone, on a spectrum of the caller's: what tests/test_gpu_mel_tail.py judges e2emel_debug_tail
against, and what tests/test_mel_tail_host.py checks and mutates.

tail_f32, float32 with one rounding per written operation:
  magnitude   mag[k] = sqrt(fl(fl(fl(re^2) + fl(im^2)) + 1e-9f)) -- the squares rounded on their own, the root correctly rounded;
  energy      lane l of 64 folds the bins l, l + 64, ... in ascending order into e = fmaf(mag, mag, e) from +0 (an exact fused multiply-add:
              fastformer_kernel_ref.fma32); the 64 partials go through the xor butterfly 32, 16, 8, 4, 2, 1, every lane adding its
              partner's value to its own (commutative, so lane 0's result is every lane's); then sqrt;
  mel         acc = the fmaf chain w[m, k] * mag[k] over the row's OWN band [first, last] (e2emel_load's first and last non-zero bin, explicit
              zeros in between included) in ascending k from +0; acc <= clip -> log_clip = fl32(log(float64(clip))), else logf(acc);
  frames >= frames[b]: exactly 0 in both outputs.
Rules: energy bit for bit; every clamp decision taken from the restated acc, clamped elements exactly log_clip; the others within K = 4 ulp of
the float64 logarithm of the restated acc (K: tests/small_ref.py's allowance for the device's logf, ASSUMED, NOT MEASURED); a NaN acc stays a
NaN, an infinite one gives +inf."""
from __future__ import annotations

import numpy as np

from aligner_ref import K_ULP
from fastformer_kernel_ref import bits, diff_count, fma32   # noqa: F401

f32, f64 = np.float32, np.float64
TAIL_MAX_FRAMES, TAIL_LDS_MAX = 16, 64 * 1024
EPS = f32(1e-9)


def tile_frames(bins):
    """Frames per workgroup: the largest power of two <= 16 whose magnitudes fit 64 KiB of LDS."""
    ft = TAIL_MAX_FRAMES
    while ft > 1 and ft * bins * 4 > TAIL_LDS_MAX:
        ft >>= 1
    return ft


def cpad_of(bins):
    return (2 * bins + 31) // 32 * 32


def band_table(basis):
    """[n_mel, 2]: first and last non-zero bin per row, (0, -1) for an all-zero row (what e2emel_load records)."""
    out = np.zeros((basis.shape[0], 2), np.int64)
    for m, row in enumerate(np.asarray(basis)):
        nz = np.flatnonzero(row)
        out[m] = (nz[0], nz[-1]) if nz.size else (0, -1)
    return out


def magnitudes(re, im, mut=None):
    """mut: "eps_outside" (the 1e-9 added to the root), "fused_squares" (fmaf(re, re, fl(im^2)))."""
    re, im = np.asarray(re, f32), np.asarray(im, f32)
    with np.errstate(all="ignore"):
        if mut == "fused_squares":
            ss = fma32(re, re, (im * im).astype(f32))
        else:
            ss = ((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)
        if mut == "eps_outside":
            return (np.sqrt(ss).astype(f32) + EPS).astype(f32)
        return np.sqrt((ss + EPS).astype(f32)).astype(f32)


def energy_of(mag, mut=None):
    """[..., bins] -> [...]; mut: "ascending" (one chain over all bins, no lane split)."""
    mag = np.asarray(mag, f32)
    bins = mag.shape[-1]
    with np.errstate(all="ignore"):
        if mut == "ascending":
            e = np.zeros(mag.shape[:-1], f32)
            for k in range(bins):
                e = fma32(mag[..., k], mag[..., k], e)
            return np.sqrt(e).astype(f32)
        lanes = np.zeros(mag.shape[:-1] + (64,), f32)
        for k0 in range(0, bins, 64):
            n = min(64, bins - k0)
            lanes[..., :n] = fma32(mag[..., k0:k0 + n], mag[..., k0:k0 + n], lanes[..., :n])
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = (lanes + lanes[..., idx ^ o]).astype(f32)
        return np.sqrt(lanes[..., 0]).astype(f32)


def band_acc(mag, basis, band, mut=None):
    """[F, bins] x [M, bins] -> acc [F, M]; mut: "band_wide" (one bin past the last), "drop_last_bin"."""
    mag, basis = np.asarray(mag, f32), np.asarray(basis, f32)
    F, bins = mag.shape
    M = basis.shape[0]
    first, last = band[:, 0].copy(), band[:, 1].copy()
    live = last >= first
    if mut == "band_wide":
        last = np.where(live, np.minimum(last + 1, bins - 1), last)
    if mut == "drop_last_bin":
        last = np.where(live, last - 1, last)
    acc = np.zeros((F, M), f32)
    width = int((last - first + 1).max()) if M else 0
    with np.errstate(all="ignore"):
        for j in range(max(width, 0)):
            rows = np.flatnonzero(first + j <= last)
            if rows.size == 0:
                break
            k = first[rows] + j
            acc[:, rows] = fma32(basis[rows, k][None, :], mag[:, k], acc[:, rows])
    return acc


def tail_f32(spec, frames, T, bins, basis, clip, mut=None):
    """spec [B, >= T, Cpad] (re | im | padding per row) -> dict(energy [B, T], acc [B, T, M], clamped [B, T, M] bool, log64 [B, T, M], live [B, T] bool,
    log_clip).  mut: magnitudes' / energy_of's / band_acc's, "lt_clamp" (acc < clip), "skip_last_frame" (frame frames[b] - 1 left unwritten:
    the caller sees whatever the buffer held, here NaN)."""
    spec = np.asarray(spec, f32)
    basis = np.asarray(basis, f32)
    B, M = spec.shape[0], basis.shape[0]
    band = band_table(basis)
    c = f32(clip)
    out = dict(energy=np.zeros((B, T), f32), acc=np.zeros((B, T, M), f32), clamped=np.zeros((B, T, M), bool), log64=np.zeros((B, T, M), f64),
               live=np.zeros((B, T), bool), log_clip=f32(np.log(f64(c))), skipped=np.zeros((B, T), bool))
    nfs = [int(min(max(frames[b], 0), T)) for b in range(B)]
    live = out["live"]
    for b, nf in enumerate(nfs):
        live[b, :nf] = True
        if mut == "skip_last_frame" and nf:
            out["skipped"][b, nf - 1] = True
    if not live.any():
        return out
    rows = spec[:, :T][live]                                     # every live frame of the batch at once: [F, Cpad]
    mag = magnitudes(rows[:, :bins], rows[:, bins:2 * bins], mut)
    out["energy"][live] = energy_of(mag, mut)
    acc = band_acc(mag, basis, band, mut)
    out["acc"][live] = acc
    with np.errstate(all="ignore"):
        out["clamped"][live] = (acc < c) if mut == "lt_clamp" else (acc <= c)
        out["log64"][live] = np.log(acc.astype(f64))
    return out


def restrict(ref, frames, T):
    """The reference of the same spectrum cut to T frames with other frame counts (a frame's results depend on its own row only)."""
    out = {k: (v[:, :T].copy() if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for k, v in ref.items()}
    live = np.zeros_like(out["live"])
    for b, nf in enumerate(frames):
        live[b, :int(min(max(nf, 0), T))] = True
    assert not np.any(live & ~out["live"])
    out["live"] = live
    out["skipped"] &= live
    for k in ("energy", "acc", "log64"):
        out[k][~live] = 0
    out["clamped"][~live] = False
    return out


def outputs_of(ref):
    """(mel, energy) the restatement itself would write, with the float64 logarithm rounded once where the kernel calls logf (within the
    rule by construction): what the host module feeds the checks with, mutated or not."""
    with np.errstate(all="ignore"):
        mel = np.where(ref["clamped"], ref["log_clip"], ref["log64"].astype(f32)).astype(f32)
    mel[~ref["live"]] = 0
    energy = ref["energy"].copy()
    mel[ref["skipped"]] = np.nan
    energy[ref["skipped"]] = np.nan
    return mel, energy


def check_tail(ref, mel, energy):
    """-> (failures, figures): the rules of the module docstring on a kernel's (mel [B, T, M], energy [B, T])."""
    mel, energy = np.asarray(mel, f32), np.asarray(energy, f32)
    fails = []
    live = ref["live"]
    nd_e = diff_count(energy, ref["energy"])
    if nd_e:
        fails.append(f"{nd_e} of {energy.size} energies differ")
    dead = np.broadcast_to(~live[:, :, None], mel.shape)
    if np.any(bits(mel)[dead] != 0) or np.any(bits(energy)[~live] != 0):
        fails.append("frames past frames[b] are not exactly 0")
    on = np.broadcast_to(live[:, :, None], mel.shape)
    cl = ref["clamped"] & on
    nd_c = int(np.count_nonzero(bits(mel)[cl] != bits(np.full(1, ref["log_clip"], f32))[0]))
    if nd_c:
        fails.append(f"{nd_c} of {int(cl.sum())} clamped elements are not exactly log_clip")
    un = ~ref["clamped"] & on
    want = ref["log64"]
    with np.errstate(all="ignore"):
        w32 = want.astype(f32)
        nan, inf = un & np.isnan(want), un & np.isinf(want)
        fin = un & np.isfinite(want)
        ulps = np.abs(mel.astype(f64) - want) / np.spacing(np.abs(w32)).astype(f64)
    bad = int(np.count_nonzero(~np.isnan(mel[nan]))) + int(np.count_nonzero(mel[inf] != w32[inf])) + int(np.count_nonzero(~(ulps[fin] <= K_ULP)))
    worst = float(ulps[fin].max()) if fin.any() else 0.0
    if bad:
        fails.append(f"{bad} of {int(un.sum())} unclamped elements off the float64 logarithm of the restated sum by more than {K_ULP} ulp (worst {worst:.3g}), or not NaN / inf where it is")
    return fails, dict(energies=int(energy.size), energies_differing=nd_e, clamped=int(cl.sum()), clamped_differing=nd_c, logs=int(un.sum()), logs_off=bad, worst_ulp=worst)
