"""Cases and seeded inputs of the small-kernel tests (tests/test_gpu_small_kernels.py, tests/test_small_ref_host.py): the smallest shapes
at which these kernels can go wrong -- H = 516 is the second trip of the 128-thread block loops (H / 4 = 129), L = 65 / 130 the second and
third 64-lane chunk of the scans, zero-length phonemes at the front, in the middle (two in a row) and at the end of a scan -- and the values
at which their decisions flip: every bucket boundary and both float32 neighbours, the fences of the duration rounding and of a dozen f0
bucket edges out to +-8 ulp, signed zeros, subnormals, infinities and NaN."""
import numpy as np

import small_ref as sr
from kernel_ref import rng_of

f32 = np.float32
CTL_FORMS = ("scalar", "utt", "phoneme")     # CtlRef: the kernel's scalar | sb = 1, sl = 0 | sb = L, sl = 1
SUBNORMAL = f32(2.0 ** -149)


def neighbours(v, k=1):
    """[v - k ulp .. v + k ulp] for every v, flattened."""
    v = np.asarray(v, f32)
    return np.concatenate([sr.nudge(v, d) for d in range(-k, k + 1)])


# ---------------------------------------------------------------- scans with zero-length phonemes
def scan_of(counts):
    return np.cumsum(np.asarray(counts, np.int64), -1).astype(np.int32)


def zero_pattern_counts(L, rng, hi=4):
    """Repeat counts of one utterance: zeros at the front, two in a row in the middle, and at the end (as far as L has room)."""
    c = rng.integers(1, hi + 1, L)
    if L >= 2:
        c[0] = 0
    if L >= 3:
        c[-1] = 0
    if L >= 6:
        c[L // 2] = c[L // 2 + 1] = 0
    return c


# ---------------------------------------------------------------- duration
DUR_SCAN_L = (1, 63, 64, 65, 130)
DUR_RANDOM = dict(B=3, L=700, lo=-2.0, hi=3.5)        # decision tier: 2 100 draws per seed
DUR_SEEDS = ("dur_a", "dur_b")


def dur_random(seed):
    c = DUR_RANDOM
    return rng_of(seed).uniform(c["lo"], c["hi"], (c["B"], c["L"])).astype(f32)


def dur_fences():
    """The float32 nearest to log(j + 1.5), j = 0 .. 20, and its neighbours out to +-8 ulp: [3, 119] (the rows repeat)."""
    v = neighbours(np.log(np.arange(21) + 1.5).astype(f32), 8)
    return np.stack([v, v[::-1], np.roll(v, 7)])


def dur_exact_inputs(L, seed):
    """log_d = log(n + 1 + offset), |offset| <= 0.2: rint gives n for every candidate of expf (far from the fences); B = 3 independent
    rows, row 1 all zero (log_d = 0: e = 0 exactly)."""
    r = rng_of(seed)
    n = r.integers(0, 6, (3, L))
    log_d = np.log(n + 1.0 + r.uniform(-0.2, 0.2, (3, L))).astype(f32)
    log_d[1] = 0.0
    return log_d


def ctl_values(form, B, L, rng, choices=(0.5, 0.75, 1.5)):
    """(values array or None, (sb, sl), scalar)."""
    if form == "scalar":
        return None, (0, 0), float(choices[0])
    if form == "utt":
        return np.asarray(rng.choice(choices, B), f32), (1, 0), 1.0
    return np.asarray(rng.choice(choices, (B, L)), f32).ravel(), (L, 1), 1.0


def ctl_of(values, strides, scalar, B, L):
    """[B, L] float32 controls a kernel sees under (values, strides) or the scalar."""
    if values is None:
        return np.full((B, L), scalar, f32)
    return sr.ctl_array((None,) + tuple(strides), values, B, L)


# ---------------------------------------------------------------- variance_embed
F0_MEAN, F0_STD = 200.0, 50.0
F0_RANDOM = dict(B=3, L=700)
F0_SEEDS = {0: ("f0_lin_a", "f0_lin_b"), 1: ("f0_log_a", "f0_log_b")}
# the edge between bucket j and j + 1.  Every edge up to 17: only there (log(1 + f0 / 700) < 1/8) are K ulp of logf narrower than the shift
# of the edges that float32-formed mel constants cause, so only there can that mutation show; a dozen more across the range
F0_FENCE_BUCKETS = tuple(range(1, 18)) + (40, 77, 101, 128, 150, 199, 230, 253, 254)


def ve_tables(H, seed="ve_tables"):
    r = rng_of(f"{seed}_{H}")
    ebins = np.linspace(-1.5, 6.0, sr.N_BINS - 1).astype(f32)                 # torch.linspace bins (U/layers.py:169)
    pbins = np.sort(r.uniform(-3.0, 3.0, sr.N_BINS - 1)).astype(f32)
    pemb = r.standard_normal((sr.N_BINS, H)).astype(f32)
    eemb = r.standard_normal((sr.N_BINS, H)).astype(f32)
    return dict(energy_bins=ebins, pitch_bins=pbins, pitch_emb=pemb, energy_emb=eemb)


def sweep(bins, ctl, rows):
    """`rows` values: bins[k] and both float32 neighbours for every k (divided by the control, so that the product lands on or next to the
    boundary), values below the first and above the last bin, +-inf, NaN, padded with the middle of the range."""
    v = np.concatenate([neighbours(bins, 1), [bins[0] - 1, bins[-1] + 1, np.inf, -np.inf, np.nan, 0.0, -0.0]]).astype(f32)
    v = (v / f32(ctl)).astype(f32)
    assert len(v) <= rows
    return np.concatenate([v, np.full(rows - len(v), v[300], f32)])


def ve_case(name, mode=2, feat=3, H=4, B=3, L=5, form="scalar", pc=1.0, ec=1.0, frame_Lp=None, kind="random"):
    """One launch: inputs + the per-row controls the kernel must apply (sr.controls_of).  Frame level (frame_Lp): L is the frame count N,
    the controls are per phoneme of a scan cum [B, Lp] with zero-length phonemes."""
    r = rng_of(name)
    d = dict(ve_tables(H), name=name, mode=mode, feat=feat, H=H, B=B, L=L, f0_mean=F0_MEAN, f0_std=F0_STD, form=form, p_scalar=pc, e_scalar=ec,
             cum=None, Lp=0, p_values=None, e_values=None, p_strides=(0, 0), e_strides=(0, 0))
    d["x"] = r.standard_normal((B, L, H)).astype(f32)
    if kind == "sweep":
        d["energy_pred"] = sweep(d["energy_bins"], ec, B * L).reshape(B, L)
        d["pitch_pred"] = sweep(d["pitch_bins"], pc, B * L).reshape(B, L)
    else:
        d["energy_pred"] = r.uniform(-2.0, 6.5, (B, L)).astype(f32)
        if mode == 2:
            d["pitch_pred"] = r.uniform(-3.5, 3.5, (B, L)).astype(f32)
        else:
            d["pitch_pred"] = np.stack([f0_pred(r.uniform(np.log(40.0), np.log(1200.0), (B, L)), mode), r.standard_normal((B, L)) - 0.5], -1).astype(f32)
    Lc = L
    if frame_Lp:
        counts = np.stack([zero_pattern_counts(frame_Lp, r, 2) for _ in range(B)])
        if frame_Lp == 1:
            counts[:] = [[L], [1], [0]][:B]
        d["cum"], d["Lp"], Lc = scan_of(counts), frame_Lp, frame_Lp
    if form != "scalar":
        d["p_values"], d["p_strides"], _ = ctl_values(form, B, Lc, r, (0.5, 0.75, 1.1, 1.5))
        d["e_values"], d["e_strides"], _ = ctl_values(form, B, Lc, r, (0.5, 0.9, 1.25))
        d["p_scalar"] = d["e_scalar"] = 7.0      # must not be used
    finish(d)
    return d


def finish(d, mut=None):
    """The per-row controls [B, N] (what the kernel must look up)."""
    B, L = d["B"], d["L"]
    for k in "pe":
        if d[k + "_values"] is None:
            d[k + "c"] = np.full((B, L), d[k + "_scalar"], f32)
        else:
            d[k + "c"] = sr.controls_of((None,) + tuple(d[k + "_strides"]), d[k + "_values"], B, L, d["cum"], mut)
    return d


def f0_pred(log_f0, mode):
    """Predictions that de-normalise to exp(log_f0) Hz: (f0 - mean) / std in mode 0, log2(f0) in mode 1."""
    f0 = np.exp(log_f0)
    return ((f0 - F0_MEAN) / F0_STD if mode == 0 else np.log2(f0)).astype(f32)


def f0_random_case(mode, seed):
    c = F0_RANDOM
    return ve_case(seed, mode=mode, feat=1, H=4, B=c["B"], L=c["L"])


def f0_fence_case(mode):
    """A dozen bucket edges (the f0 at which the scaled mel is j + 0.5) as predictions, with neighbours out to +-8 ulp, and the exact ends of
    the coding: f0d = -700 (mode 0: log(0), bucket 1), f0d <= 0, uv set, a huge f0 and +inf (bucket 255), NaN (any index in the table)."""
    j = np.asarray(F0_FENCE_BUCKETS, np.float64)
    mel = sr.F0_MEL_MIN + (j - 0.5) * (sr.F0_MEL_MAX - sr.F0_MEL_MIN) / 254.0
    edges = neighbours(f0_pred(np.log(700.0 * (np.exp(mel / 1127.0) - 1.0)), mode), 8)
    ends = [(-18.0, -1.0), (-4.0, -1.0), (-30.0, -1.0), (1.0, 0.5), (1.0e30, -1.0), (np.inf, -1.0), (np.nan, -1.0), (1.0, np.nan), (-np.inf, -1.0)]
    if mode == 1:
        ends = [(-200.0, -1.0), (-np.inf, -1.0), (1.0, 0.5), (100.0, -1.0), (np.inf, -1.0), (np.nan, -1.0), (8.0, np.nan), (130.0, -1.0)]
    n = len(edges) + len(ends)
    L = (n + 2) // 3
    d = ve_case(f"f0_fence_{mode}", mode=mode, feat=1, H=4, B=3, L=L)
    pp = d["pitch_pred"].reshape(-1, 2)
    pp[:len(edges), 0], pp[:len(edges), 1] = edges, -1.0
    pp[len(edges):n] = np.asarray(ends, f32)
    d["n_ends"], d["n_edges"] = len(ends), len(edges)
    return d


def uv_case():
    """The uv rule `> 0` at +0.0, -0.0, the smallest positive subnormal reached as a product that underflows to it, its negative, and
    ordinary values of either sign; per-phoneme controls (the product 2^-75 * 2^-74 = 2^-149)."""
    d = ve_case("uv_signs", mode=0, feat=1, H=4, B=3, L=2, form="phoneme")
    uv = np.asarray([0.0, -0.0, 2.0 ** -75, -(2.0 ** -75), 0.25, -0.25], f32)
    ctl = np.asarray([1.5, 1.5, 2.0 ** -74, 2.0 ** -74, 1.5, 0.75], f32)
    d["pitch_pred"][..., 1] = uv.reshape(3, 2)
    d["pitch_pred"][..., 0] = f32(1.0) / ctl.reshape(3, 2)        # f0 * control = 1 (250 Hz)
    d["pitch_pred"][1, :, 0] = 1.0                                # under the tiny controls: f0 = 2^-74 (200 Hz)
    d["p_values"] = ctl
    return finish(d)


VE_GEOMETRY = [   # (mode, feat, H, L, form)
    (2, 3, 4, 1, "scalar"), (2, 3, 256, 5, "utt"), (2, 3, 516, 5, "phoneme"), (2, 1, 516, 1, "phoneme"), (2, 2, 256, 5, "scalar"),
    (0, 3, 516, 5, "utt"), (0, 1, 4, 5, "phoneme"), (0, 2, 516, 1, "utt"), (1, 3, 256, 1, "scalar"), (1, 1, 516, 5, "scalar"),
]
VE_FRAME = [(2, 1, 9, "phoneme"), (2, 6, 9, "phoneme"), (0, 6, 7, "phoneme"), (2, 6, 1, "utt")]    # (mode, Lp, N frames, form)


def ve_geometry_case(mode, feat, H, L, form):
    pc, ec = (0.75, 1.1) if form == "scalar" else (1.0, 1.0)
    return ve_case(f"ve_{mode}_{feat}_{H}_{L}_{form}", mode=mode, feat=feat, H=H, L=L, form=form, pc=pc, ec=ec)


def ve_frame_case(mode, Lp, N, form):
    return ve_case(f"ve_frame_{mode}_{Lp}_{N}_{form}", mode=mode, feat=3, H=4, L=N, form=form, frame_Lp=Lp)


def ve_sweep_case(pc, ec):
    return ve_case(f"ve_sweep_{pc}_{ec}", mode=2, feat=3, H=4, B=3, L=260, pc=pc, ec=ec, kind="sweep")


# ---------------------------------------------------------------- length regulator
LR_CASES = [(1, 5, 4), (7, 40, 256), (70, 300, 516), (7, 33, 516)]      # (L, T, H), B = 3


def lr_data(L, T, H):
    """B = 3: an utterance with mel_len = 0, one with mel_len = T whose scan ends below T (the teacher's mel_given case: the frames past
    the total take phoneme L - 1), one whose scan total is its mel_len."""
    r = rng_of(f"lr_{L}_{T}_{H}")
    counts = np.stack([zero_pattern_counts(L, r, max(1, min(6, T // max(L, 1)))) for _ in range(3)])
    if L == 1:
        counts[:, 0] = [3, 2, 1]
    cum = scan_of(counts)
    total = cum[:, -1]
    mel = np.array([0, T, min(int(total[2]), T)], np.int32)
    assert total[1] < T
    return dict(x=r.standard_normal((3, L, H)).astype(f32), cum=cum, mel=mel, pos=r.standard_normal((T, H)).astype(f32))


# ---------------------------------------------------------------- predictor positions
VP_CASES = [(1, 4), (64, 516), (65, 4), (129, 516)]       # (L, H), B = 3


def vp_data(L, H):
    """Column 0: row 0 has -0.0 (zero), NaN and subnormals (nonzero) among ordinary values and zeros, row 1 is all zero, row 2 has no zeros."""
    r = rng_of(f"vp_{L}_{H}")
    x = r.standard_normal((3, L, H)).astype(f32)
    col = x[0, :, 0]
    col[r.random(L) < 0.4] = 0.0
    for i, v in enumerate((-0.0, np.nan, SUBNORMAL, -SUBNORMAL)):
        if i < L:
            col[(i * 17) % L] = v
    x[1, :, 0] = 0.0
    table = r.standard_normal((L + 1, H)).astype(f32)      # table_rows = L + 1 exactly
    return dict(x=x, table=table, alpha=f32(0.3), x2=r.standard_normal((3, L, H)).astype(f32))


# ---------------------------------------------------------------- the remaining exact kernels
EMBED_CASES = [(3, 5, 4), (3, 1, 256), (2, 7, 516)]       # (B, L, H)
ACT_ROWS_B = (1, 64, 65)
ACCUM_CASES = [(n, with_k, div) for n in (4, 1028) for with_k in (False, True) for div in (1.0, 3.0)]
TRANSPOSE_CT = (1, 31, 32, 33, 80)
REFLECT_CASES = [(n, C) for n in (2, 3, 257) for C in (4, 20)]
ROWDOT_CASES = [(C, O, lens) for C in (4, 256, 260, 1028) for O in (1, 2) for lens in (False, True)]
ISTFT_CASES = [(16, 4, 2), (16, 4, 9), (16, 4, 70), (4, 1, 3), (4, 2, 5), (8, 4, 70), (256, 64, 5)]      # (n_fft, hop, F), B = 2


def istft_data(nfft, hop, F, pad=0):
    """q [2, F, 2 bins + pad]: log-magnitudes low enough that |wav| stays far inside (-1, 1) and that the share of samples within the
    bar of a PCM rounding boundary stays under 0.1 % (the share is about 2 x 32768 x bar; checked on the CPU), phase arguments in
    (-3, 3); the pad columns are NaN."""
    r = rng_of(f"istft_{nfft}_{hop}_{F}")
    bins = nfft // 2 + 1
    q = np.full((2, F, 2 * bins + pad), np.nan, f32)
    q[..., :bins] = r.uniform(-9.0, -7.0, (2, F, bins))
    q[..., bins:2 * bins] = r.uniform(-3.0, 3.0, (2, F, bins))
    return q
