"""Plain-numpy references of the integer-decision and index kernels of csrc/small_kernels.hip (embedding, speaker add, predictor positions,
rowdot, duration, variance_embed, the length regulator, act_rows, the join, the transpose, the iSTFT tail) and the criteria their outputs
are judged by.  Imported by tests/test_gpu_small_kernels.py (the kernel's output goes through check_*) and tests/test_small_ref_host.py (a
mutated restatement goes through the same check_* and must fail).  Nothing here runs the reference project's code; its functions are
cited by file and line, as the kernels cite them.

Three tiers.
  Exact: no transcendental on the path.  The reference is the kernel's contract restated one float32 rounding per operation; every element
    must hold its bits.
  Decision: a transcendental (expf, logf, powf) precedes an integer decision.  The restatement is evaluated with the transcendental's
    result replaced by each of 2 K + 1 candidates -- the float64 value rounded to float32, moved by -K .. +K ulp.  An element on which all
    candidates decide alike is DECIDED and must match; any other must take one of the candidates' decisions.  K = 4 is ASSUMED to bound
    the device functions' error: the HIP math documentation was not at hand when this was written, and K is not fitted to a kernel's
    output.  What follows a decision (the scan of the repeat counts, the embedding rows added) is restated from the kernel's own
    decision, exactly.
  Bars: continuous results against float64, per element: gamma_n S (kernel_ref.gamma), plus for the iSTFT 4 x the deviation of a float32
    restatement measured on the same inputs.

Every check_* returns a list of failure strings (empty: passed) and never looks at anything but its arguments."""
import numpy as np

from kernel_ref import AGG_FACTOR, gamma, pcm_boundary, pcm_of   # noqa: F401

f32 = np.float32
K_ULP = 4                    # assumed maximum ulp error of expf / logf / powf / sinf / cosf on the device (see above)
CAP = 1048576.0              # 2^20 frames per phoneme (csrc/small_kernels.hip: duration_kernel)
I32MAX = 2 ** 31 - 1
N_BINS = 256                 # the only bin count launch_variance_embed admits (reference U/function.py:9)
F0_MEL_MIN = 1127.0 * np.log(1.0 + 50.0 / 700.0)     # U/function.py:12-13: float64 constants
F0_MEL_MAX = 1127.0 * np.log(1.0 + 1100.0 / 700.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def same_bits(a, b):
    """Bit for bit; two NaNs count as the same whatever their payloads."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    eq = bits(a) == bits(b)
    if a.dtype.kind == "f":
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(np.all(eq))


def nudge(v, d):
    """float32 array moved by d ulp (d < 0: towards -inf); zeros, infinities and NaN stay (an error of k ulp is relative)."""
    v = np.asarray(v, f32)
    out = v.copy()
    for _ in range(abs(int(d))):
        out = np.nextafter(out, f32(np.inf if d > 0 else -np.inf), dtype=f32)
    keep = (v == 0) | ~np.isfinite(v)
    return np.where(keep, v, out).astype(f32)


def candidates(t64, k=K_ULP):
    """[2 k + 1, ...]: the float64 result of a transcendental rounded to float32, moved by -k .. +k ulp."""
    with np.errstate(over="ignore", invalid="ignore"):
        c0 = np.asarray(t64, np.float64).astype(f32)
    return np.stack([nudge(c0, d) for d in range(-k, k + 1)])


def ctl_array(form, values, B, L):
    """The control of element (b, l) under CtlRef (p, sb, sl) over `values` (csrc/kernels.h): [B, L] float32."""
    p, sb, sl = form
    v = np.asarray(values, f32).ravel()
    b, l = np.meshgrid(np.arange(B), np.arange(L), indexing="ij")
    return v[b * sb + l * sl]


def frame_phoneme(cum, T, mut=None):
    """[B, T]: the smallest i with cum[b, i] > t, Lp - 1 when there is none (the binary search of length_regulate_kernel / variance_embed_kernel)."""
    B, Lp = cum.shape
    t = np.arange(T)
    gt = cum[:, None, :] > t[None, :, None]                       # [B, T, Lp]
    if mut == "frame_largest":
        idx = np.where(gt.any(-1), Lp - 1 - np.argmax(gt[..., ::-1], -1), Lp - 1)
    else:
        idx = np.where(gt.any(-1), np.argmax(gt, -1), Lp - 1)
    return idx


# ---------------------------------------------------------------- duration (reference U/layers.py:218-221, 448-449)
def duration_candidates(log_d, ctl, k=K_ULP, mut=None):
    """[2 k + 1, B, L] float32: dur = max(rint(expf(log_d) - 1) * ctl, 0) for every candidate of expf; the sign of a zero is not part of the
    contract (fmaxf(-0.0, 0.0) may be either; + 0.0 folds them here and in the check)."""
    with np.errstate(over="ignore", invalid="ignore"):
        c = candidates(np.exp(np.asarray(log_d, f32).astype(np.float64)), k)
        e = (c - f32(1.0)).astype(f32)
        if mut == "half_up":
            r = np.floor((e + f32(0.5)).astype(f32))
        elif mut == "trunc_round":
            r = np.trunc(e)
        elif mut == "shift_one":
            r = np.floor(e) + f32(1.0)
        else:
            r = np.rint(e)
        if mut == "clamp_first":
            d = (np.fmax(r, f32(0.0)) * ctl[None]).astype(f32)
            d = np.where(np.isnan(d), f32(0.0), d)
        else:
            d = np.fmax((r * ctl[None]).astype(f32), f32(0.0))     # fmax drops a NaN operand: dur of NaN is 0 (csrc/kernels.h)
    return (d + f32(0.0)).astype(f32)


def duration_scan(dur, mut=None):
    """From durations to (counts, cum int32 [B, L], mel64, mel32): count = trunc(min(dur, 2^20)), 0 for NaN; inclusive scan, cum and mel32
    saturated at 2^31 - 1, mel64 not."""
    d = np.asarray(dur, f32)
    with np.errstate(invalid="ignore"):
        capped = d if mut == "no_cap" else np.minimum(d, f32(CAP))
        capped = np.where(np.isnan(d), 0.0, np.minimum(capped.astype(np.float64), 2.0 ** 40))
    cnt = (np.rint(capped) if mut == "round_count" else np.trunc(capped)).astype(np.int64)
    cum = np.cumsum(cnt, 1)
    if mut == "no_carry":
        for l0 in range(64, cum.shape[1], 64):
            cum[:, l0:l0 + 64] = np.cumsum(cnt[:, l0:l0 + 64], 1)
    total = cum[:, -1].copy()
    if mut == "exclusive":
        cum = cum - cnt
    return cnt, np.minimum(cum, I32MAX).astype(np.int32), total, np.minimum(total, I32MAX).astype(np.int32)


def duration_ref(log_d, ctl, mut=None):
    """The nominal evaluation (candidate 0 ulp): dict(dur, cum, mel64, mel32)."""
    c = duration_candidates(log_d, ctl, mut=mut)
    dur = c[c.shape[0] // 2]
    _, cum, m64, m32 = duration_scan(dur, mut)
    return dict(dur=dur, cum=cum, mel64=m64, mel32=m32)


def check_duration(got, log_d, ctl, k=K_ULP):
    """(failures, undecided mask)."""
    c = duration_candidates(log_d, ctl, k)
    g = (np.asarray(got["dur"], f32) + f32(0.0)).astype(f32)
    hit = (bits(c) == bits(g)[None]).any(0)
    undecided = (bits(c) != bits(c[0])[None]).any(0)
    fails = []
    if not hit.all():
        i = tuple(np.argwhere(~hit)[0])
        fails.append(f"dur{i} = {g[i]!r} is none of the candidates' decisions {sorted(set(c[(slice(None),) + i].tolist()))} (log_d {log_d[i]!r}, control {ctl[i]!r})")
    _, cum, m64, m32 = duration_scan(g)
    for name, want in (("cum", cum), ("mel64", m64), ("mel32", m32)):
        if not np.array_equal(np.asarray(got[name]), want):
            j = tuple(np.argwhere(np.asarray(got[name]) != want)[0])
            fails.append(f"{name}{j} = {np.asarray(got[name])[j]} != {want[j]} (the scan of the kernel's own durations)")
    return fails, undecided


# ---------------------------------------------------------------- variance_embed (reference U/layers.py:136-171, U/function.py:178-187)
def bucketize(bins, v, mut=None):
    """First index whose boundary is >= v (torch.bucketize, right = False); NaN sorts past the last boundary, there as here."""
    return np.searchsorted(np.asarray(bins, f32), np.asarray(v, f32), side="right" if mut == "le_search" else "left").astype(np.int32)


def _flush(v):
    return np.where(np.abs(v) < np.finfo(f32).tiny, f32(0.0) * np.sign(v), v).astype(f32)


def f0_decisions(f0, uvl, mode, f0_mean, f0_std, k=K_ULP, mut=None):
    """[n_cand, ...] int32 bucket of every candidate evaluation (-1: the index is unspecified -- NaN reached the integer cast), for
    f0 / uvl already multiplied by the control.  Mode 0: logf's candidates; mode 1: powf's x logf's."""
    f0, uvl = np.asarray(f0, f32), np.asarray(uvl, f32)
    mel_min, mel_range = f32(F0_MEL_MIN), f32(F0_MEL_MAX - F0_MEL_MIN)
    if mut == "mel_consts32":
        mel_min = (f32(1127.0) * np.log(f32(1.0) + f32(50.0) / f32(700.0))).astype(f32)
        mel_range = f32((f32(1127.0) * np.log(f32(1.0) + f32(1100.0) / f32(700.0))).astype(f32) - mel_min)
    with np.errstate(all="ignore"):
        if mode == 1 and mut != "mode1_as_0":
            f0ds = candidates(np.exp2(f0.astype(np.float64)), k)
        else:
            f0ds = ((f0 * f32(f0_std)).astype(f32) + f32(f0_mean)).astype(f32)[None]
        out = []
        for f0d in f0ds:
            f0d = np.where((uvl >= 0) if mut == "uv_ge" else (uvl > 0), f32(0.0), f0d).astype(f32)
            a = (f32(1.0) + (f0d / f32(700.0)).astype(f32)).astype(f32)
            for lg in candidates(np.log(a.astype(np.float64)), k):
                mel = (f32(1127.0) * lg).astype(f32)
                if mut == "plus_one_first":
                    sc = ((((mel - mel_min).astype(f32) + f32(1.0)).astype(f32) * f32(254.0)).astype(f32) / mel_range).astype(f32)
                else:
                    sc = ((((mel - mel_min).astype(f32) * f32(254.0)).astype(f32) / mel_range).astype(f32) + f32(1.0)).astype(f32)
                mel = np.where(mel > 0, sc, mel)
                mel = np.where(mel <= 1, f32(1.0), mel)
                mel = np.where(mel > 255, f32(255.0), mel).astype(f32)
                v = mel if mut == "no_half" else (mel + f32(0.5)).astype(f32)
                idx = np.where(np.isnan(v), -1, np.trunc(np.nan_to_num(v)).astype(np.int64))
                out.append(np.where(idx < 0, idx, np.clip(idx, 0, N_BINS - 1)).astype(np.int32))
    return np.stack(out)


def variance_embed_ref(d, mut=None):
    """The nominal evaluation of one launch.  d: x [B, N, H], pitch_pred ([B, N, 2], mode 2: [B, N]), energy_pred [B, N], pc / ec [B, N]
    (controls per row, already looked up -- see controls_of), f0_mean, f0_std, energy_bins, pitch_bins, pitch_emb, energy_emb, mode, feat.
    Returns dict(x, pitch_pred, pitch_idx, energy_idx); an index array of an absent feature is None (the kernel leaves it alone)."""
    mode, feat = d["mode"], d["feat"]
    pc, ec = d["pc"], d["ec"]
    pp = np.array(d["pitch_pred"], f32)
    pidx = eidx = None
    if feat & 1:
        if mode == 2:
            v = pp if mut == "ctl_after_bucket" else (pp * pc).astype(f32)
            pidx = bucketize(d["pitch_bins"], v, mut)
        else:
            f0, uvl = (pp[..., 0] * pc).astype(f32), (pp[..., 1] * pc).astype(f32)
            if mut == "flush_subnormal":
                f0, uvl = _flush(f0), _flush(uvl)
            dec = f0_decisions(f0, uvl, mode, d["f0_mean"], d["f0_std"], mut=mut)
            pidx = np.maximum(dec[dec.shape[0] // 2], 0)
            pp = np.stack([f0, uvl], -1)
    if feat & 2:
        v = d["energy_pred"] if mut == "ctl_after_bucket" else (d["energy_pred"] * ec).astype(f32)
        eidx = bucketize(d["energy_bins"], v, mut)
    x = embed_add(d, pidx, eidx, mut)
    if mut == "wrong_feature_idx" and feat == 3:
        pidx, eidx = eidx, pidx
    return dict(x=x, pitch_pred=pp, pitch_idx=pidx, energy_idx=eidx)


def embed_add(d, pidx, eidx, mut=None):
    """x = (x + pitch_emb[pidx]) + energy_emb[eidx] in float32, or the single add of the one feature present."""
    x = np.asarray(d["x"], f32)
    if d["feat"] == 3:
        if mut == "ee_first":
            return ((x + d["energy_emb"][eidx]).astype(f32) + d["pitch_emb"][pidx]).astype(f32)
        return ((x + d["pitch_emb"][pidx]).astype(f32) + d["energy_emb"][eidx]).astype(f32)
    return (x + (d["pitch_emb"][pidx] if d["feat"] & 1 else d["energy_emb"][eidx])).astype(f32)


def controls_of(form, values, B, N, cum=None, mut=None):
    """[B, N] controls of a variance_embed pass: phoneme level (cum None) element (b, t) takes CtlRef element (b, t); frame level it
    takes element (b, frame_phoneme(cum)[b, t])."""
    p, sb, sl = form
    v = np.asarray(values, f32).ravel()
    b = np.arange(B)[:, None]
    l = np.arange(N)[None, :] if cum is None else frame_phoneme(cum, N, mut)
    return v[b * sb + l * sl]


def check_variance_embed(got, d, sentinel_idx, k=K_ULP):
    """got: dict(x, pitch_pred, pitch_idx, energy_idx) as the kernel left them (index arrays pre-filled with sentinel_idx).
    Returns (failures, undecided mask or None)."""
    mode, feat = d["mode"], d["feat"]
    fails, undecided = [], None
    pp0 = np.asarray(d["pitch_pred"], f32)
    gp, ge = np.asarray(got["pitch_idx"]), np.asarray(got["energy_idx"])
    if not feat & 1:
        if not np.all(gp == sentinel_idx):
            fails.append("pitch_idx written although the pitch takes no part")
        if not same_bits(got["pitch_pred"], pp0):
            fails.append("pitch_pred changed although the pitch takes no part")
    elif mode == 2:
        if not same_bits(got["pitch_pred"], pp0):
            fails.append("mode 2: pitch_pred must keep its bits")
        want = bucketize(d["pitch_bins"], (pp0 * d["pc"]).astype(f32))
        if not np.array_equal(gp, want):
            i = tuple(np.argwhere(gp != want)[0])
            fails.append(f"pitch_idx{i} = {gp[i]} != {want[i]} (value {(pp0 * d['pc']).astype(f32)[i]!r})")
    else:
        f0, uvl = (pp0[..., 0] * d["pc"]).astype(f32), (pp0[..., 1] * d["pc"]).astype(f32)
        if not same_bits(got["pitch_pred"], np.stack([f0, uvl], -1)):
            fails.append("pitch_pred does not hold the two float32 products prediction * control")
        dec = f0_decisions(f0, uvl, mode, d["f0_mean"], d["f0_std"], k)
        free = (dec < 0).any(0)
        undecided = (dec != dec[0][None]).any(0) & ~free
        ok = (dec == gp[None]).any(0) | (free & (gp >= 0) & (gp <= N_BINS - 1))
        if not ok.all():
            i = tuple(np.argwhere(~ok)[0])
            fails.append(f"pitch_idx{i} = {gp[i]} is none of the candidates' decisions {sorted(set(dec[(slice(None),) + i].tolist()))} (f0 {f0[i]!r}, uv {uvl[i]!r})")
    if not feat & 2:
        if not np.all(ge == sentinel_idx):
            fails.append("energy_idx written although the energy takes no part")
    else:
        want = bucketize(d["energy_bins"], (d["energy_pred"] * d["ec"]).astype(f32))
        if not np.array_equal(ge, want):
            i = tuple(np.argwhere(ge != want)[0])
            fails.append(f"energy_idx{i} = {ge[i]} != {want[i]} (value {(d['energy_pred'] * d['ec']).astype(f32)[i]!r})")
    if not fails:   # the rows added are those of the kernel's own (admissible) indices
        want = embed_add(d, gp if feat & 1 else None, ge if feat & 2 else None)
        if not same_bits(got["x"], want):
            fails.append("x is not x + the embedding rows of the indices written, in float32 and in the kernel's order")
    return fails, undecided


# ---------------------------------------------------------------- length regulator (reference U/layers.py:429-451)
def length_regulate_ref(x, cum, mel_lens, pos, T, mut=None):
    """np.repeat of the phoneme rows by the scan's differences, frames past the scan total (mel_len given from outside) take phoneme
    L - 1, rows at or past mel_len are zero; + pos[t] in one float32 add on every row when pos is given."""
    B, L, H = x.shape
    y = np.zeros((B, T, H), f32)
    for b in range(B):
        cnt = np.diff(np.concatenate([[0], cum[b].astype(np.int64)]))
        rows = np.repeat(np.arange(L), cnt)[:T]
        rows = np.concatenate([rows, np.full(T - len(rows), L - 1, np.int64)]).astype(np.int64)
        if mut == "frame_largest":
            rows = frame_phoneme(cum[b:b + 1], T, mut)[0]
        n = int(min(max(mel_lens[b], 0), T))
        y[b, :n] = x[b, rows[:n]]
    if pos is not None:
        y = (y + pos[None, :T]).astype(f32)
    return y


# ---------------------------------------------------------------- predictor positions (reference U/function.py:28-38, U/layers.py:497-498)
def var_positions_ref(x, table, alpha, posbuf=None, mut=None):
    """(positions int32 [B, L], y): positions = cumsum(x[..., 0] != 0) * (x[..., 0] != 0); y = x + fl(alpha * table[pos]), two roundings."""
    if posbuf is None:
        nz = (x[..., 0] != 0).astype(np.int64)
        c = np.cumsum(nz, 1)
        if mut == "no_carry":
            for l0 in range(64, c.shape[1], 64):
                c[:, l0:l0 + 64] = np.cumsum(nz[:, l0:l0 + 64], 1)
        posbuf = (c * nz).astype(np.int32)
    rows = table[np.minimum(posbuf, table.shape[0] - 1)]
    if mut == "fma":
        y = (x.astype(np.float64) + np.float64(alpha) * rows.astype(np.float64)).astype(f32)    # one rounding (the product is exact in float64)
    else:
        y = (x + (f32(alpha) * rows).astype(f32)).astype(f32)
    return posbuf, y


# ---------------------------------------------------------------- the remaining exact kernels
def embed_ref(ids, emb, pos):
    B, L = ids.shape
    return (emb[np.clip(ids, 0, emb.shape[0] - 1)] + pos[None, :L]).astype(f32)


def add_speaker_ref(xin, spk, speaker):
    B = xin.shape[0]
    sid = np.clip(np.asarray(speaker, np.int64), 0, spk.shape[0] - 1)
    sid = np.full(B, sid[0]) if len(sid) == 1 else sid
    return (xin + spk[sid][:, None, :]).astype(f32)


def act_rows_ref(lens, add, mul, cap, add_rows=0):
    v = (np.asarray(lens, np.int64) + add) * mul + add_rows
    return np.minimum(v, cap).astype(np.int32)


def accum_div_ref(S, Sj, Sk, div):
    a = (S + Sj).astype(f32)
    if Sk is not None:
        a = (a + Sk).astype(f32)
    return (a / f32(div)).astype(f32) if div != 1.0 else a


def reflect_lrelu_ref(x, slope):
    """[B, n, C] -> [B, n + 1, C]: frame 0 of the padded signal is frame 1 of the input (ReflectionPad1d((1, 0))); max(v, v * slope)."""
    v = np.maximum(x, (x * f32(slope)).astype(f32))
    return np.concatenate([v[:, 1:2], v], 1)


def rowdot_ref(x, w, b, lens, L):
    """(out float64 [rows, O], bar): dot + bias; rows at or past lens[b] are exactly 0 (bar 0)."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    out = x64 @ w64.T + b.astype(np.float64)
    S = np.abs(x64) @ np.abs(w64).T + np.abs(b.astype(np.float64))
    bar = gamma(x.shape[1] + 1) * S
    if lens is not None:
        r = np.arange(x.shape[0])
        masked = (r % L) >= np.asarray(lens)[r // L]
        out[masked], bar[masked] = 0.0, 0.0
    return out, bar


# ---------------------------------------------------------------- iSTFT tail (reference V/generator.py:107-113, src/tools/stft.py:138-148)
def istft_bar_n(nfft, hop, k=K_ULP):
    """Roundings on the path of one term of a sample: the k-sum and the two edge bins (2 bins), the frame sums of numerator and
    denominator (2 n_fft / hop), product, 1/N, w, w^2, the division and slack (8); and, at up to 2 k ulp between two implementations of a
    transcendental, expf (1), cos / sin of a phase that is itself sinf's result (1 + tan(1) < 2.6), the twiddle (1) and the window's
    cosine in numerator and denominator (3): 2 k x 8 in round figures."""
    return 2 * (nfft // 2 + 1) + 2 * (nfft // hop) + 8 + 16 * k


def istft_eval(q, nfft, hop, dtype=np.float64, mut=None):
    """torch.istft(spec * exp(j phase), n_fft, hop, window = hann_window(n_fft) [periodic], center = True) from q [B, F, >= 2 bins]
    (spec = exp(q[:bins]), phase = sin(q[bins:2 bins])), by the definition.  float64: the reference.  float32: the kernel's operations
    restated (angle, twiddles and window formed in float32; k, then frames, summed in order).  Returns dict(specphase, wav, S, den)."""
    B, F = q.shape[:2]
    bins, N = nfft // 2 + 1, nfft
    t = dtype
    qq = q[..., :2 * bins].astype(t)
    spec, phase = np.exp(qq[..., :bins]).astype(t), np.sin(qq[..., bins:]).astype(t)
    re, im = (spec * np.cos(phase).astype(t)).astype(t), (spec * np.sin(phase).astype(t)).astype(t)
    m = np.arange(N)
    if t is np.float64:
        a = 2.0 * np.pi * m / N
    else:
        a = ((f32(6.283185307179586) * m.astype(f32)).astype(f32) / f32(N)).astype(f32)
    cs, sn = np.cos(a).astype(t), np.sin(a).astype(t)
    if mut == "sym_hann":
        win = (t(0.5) - t(0.5) * np.cos(2.0 * np.pi * m / (N - 1))).astype(t)
    else:
        win = (t(0.5) - (t(0.5) * cs).astype(t)).astype(t)
    # Y[b, f, m]: the real inverse DFT of frame f at m, before the 1 / N; Ya: the same sum over absolute values (for the bar)
    sg = np.where(m & 1, -1.0, 1.0).astype(t) if mut != "nyquist_sign" else np.ones(N, t)
    Y = ((re[..., 0:1] * t(2.0 if mut == "dc_doubled" else 1.0)).astype(t) + (sg * re[..., bins - 1:bins]).astype(t)).astype(t)
    Y = np.broadcast_to(Y, (B, F, N)).copy()
    Ya = np.broadcast_to(np.abs(re[..., 0:1]) + np.abs(re[..., bins - 1:bins]), (B, F, N)).astype(np.float64).copy()
    for k in range(1, bins - 1):
        idx = (k * m) & (N - 1)
        term = ((re[..., k:k + 1] * cs[idx]).astype(t) - (im[..., k:k + 1] * sn[idx]).astype(t)).astype(t)
        Y = (Y + (t(2.0) * term).astype(t)).astype(t)
        Ya += 2.0 * (np.abs(re[..., k:k + 1] * cs[idx]) + np.abs(im[..., k:k + 1] * sn[idx]))
    if mut != "no_1_over_n":
        Y = (Y / t(N)).astype(t)
    Ya = Ya / N
    nsamp = hop * (F - 1)
    n = np.arange(nsamp)
    np_ = n + N // 2 + (1 if mut == "trim_off_by_one" else 0)
    f_hi = np.minimum(np_ // hop, F - 1)
    f_lo = np.maximum((np_ - N + hop) // hop, 0)
    if mut == "drop_first_frame":
        f_lo = np.where(f_hi > f_lo, f_lo + 1, f_lo)
    if mut == "drop_last_frame":
        f_hi = np.where(f_hi > f_lo, f_hi - 1, f_hi)
    num, den, S = np.zeros((B, nsamp), t), np.zeros(nsamp, t), np.zeros((B, nsamp))
    for r in range(N // hop + 1):
        f = f_lo + r
        ok = f <= f_hi
        fc = np.where(ok, f, 0)
        mm = np.clip(np_ - fc * hop, 0, N - 1)
        w = np.where(ok, win[mm], t(0.0)).astype(t)
        num = (num + (w * Y[:, fc, mm]).astype(t)).astype(t)
        den = (den + (w * w).astype(t)).astype(t)
        S += np.abs(w) * Ya[:, fc, mm]
    with np.errstate(divide="ignore", invalid="ignore"):
        wav = (num / den).astype(t)
    return dict(specphase=np.concatenate([spec, phase], -1), wav=wav, S=S, den=den.astype(np.float64))


def ulp_of(v64):
    """Spacing of float32 at |v| (of the binade of v rounded to float32)."""
    a = np.abs(np.asarray(v64, np.float64)).astype(f32)
    return (np.nextafter(a, f32(np.inf), dtype=f32).astype(np.float64) - a.astype(np.float64))


def istft_reference(q, nfft, hop):
    """dict(specphase64, wav64, bar, dev, ...): the float64 definition, the per-sample bar gamma_n S / den + 4 x |float32 restatement - float64|."""
    r64, r32 = istft_eval(q, nfft, hop, np.float64), istft_eval(q, nfft, hop, f32)
    dev = np.abs(r32["wav"].astype(np.float64) - r64["wav"])
    lin = gamma(istft_bar_n(nfft, hop)) * r64["S"] / r64["den"]
    return dict(specphase=r64["specphase"], wav=r64["wav"], lin=lin, dev=dev, bar=lin + AGG_FACTOR * dev, wav32=r32["wav"])


def check_istft(got, ref, k=K_ULP):
    """got: dict(specphase float32 or None-less, wav float32 or None, pcm int16 or None).  Returns (failures, figures)."""
    fails, fig = [], {}
    sp = np.asarray(got["specphase"], f32)
    e = np.abs(sp.astype(np.float64) - ref["specphase"]) / ulp_of(ref["specphase"])
    fig["specphase_ulp"] = float(e.max())
    if not e.max() <= k:
        fails.append(f"specphase: {e.max():.2f} ulp from the float64 value (allowed {k})")
    wav = got.get("wav")
    if wav is not None:
        wav = np.asarray(wav, f32)
        if not np.all(np.isfinite(wav)):
            fails.append("wav: not finite")
        else:
            ratio = np.abs(wav.astype(np.float64) - ref["wav"]) / ref["bar"]
            fig["wav_ratio"] = float(ratio.max())
            if not ratio.max() <= 1.0:
                i = tuple(np.argwhere(ratio > 1.0)[0])
                fails.append(f"wav{i}: err / bar = {ratio[i]:.3g} ({wav[i]!r} against {ref['wav'][i]!r})")
    pcm = got.get("pcm")
    if pcm is not None:
        pcm = np.asarray(pcm, np.int16)
        if wav is not None and not np.array_equal(pcm, pcm_of(wav)):
            fails.append("pcm is not (int16)(int32)(wav * 32768) of the kernel's own wav")
        want = np.trunc(ref["wav"] * 32768.0).astype(np.int64)
        excl = pcm_boundary(ref["wav"], ref["bar"])
        fig["pcm_excluded"] = float(excl.mean())
        diff = np.abs(pcm.astype(np.int64) - want)
        if not excl.mean() <= 1e-3:
            fails.append(f"pcm: {excl.mean():.2%} of the samples lie at a rounding boundary (allowed 0.1 %)")
        if np.any(diff[~excl] != 0):
            fails.append(f"pcm: {int(np.sum(diff[~excl] != 0))} samples off the rounding boundaries differ from the reference")
        if diff.max() > 1:
            fails.append(f"pcm: {diff.max()} LSB from the reference")
    return fails, fig
