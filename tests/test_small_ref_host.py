"""CPU checks of what tests/test_gpu_small_kernels.py relies on (tests/small_ref.py, tests/small_cases.py):
  - the references against independent evaluations (torch.bucketize, torch.round, torch.cumsum, numpy's searchsorted / irfft, float64
    torch.istft, float64 formulas);
  - the caps, on the reference alone: the undecided share of the seeded random elements (<= 1e-3, pooled per family) and the share of
    iSTFT samples at a PCM rounding boundary (<= 0.1 % per case);
  - mutations: every listed mutation of a restatement fails the GPU test's own criterion (small_ref.check_*) at a small case;
  - every refusal of the launch wrappers (they return before launching, so this needs no GPU)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import small_cases as sc   # noqa: E402
import small_ref as sr     # noqa: E402

f32 = np.float32
ISENT = -777


# ---------------------------------------------------------------- references against independent evaluations
def test_bucketize_is_torch_bucketize_at_every_boundary_and_on_the_specials():
    import torch
    for pc, ec in ((1.0, 1.0), (0.75, 1.1)):
        d = sc.ve_sweep_case(pc, ec)
        for bins, v in ((d["energy_bins"], (d["energy_pred"] * d["ec"]).astype(f32)), (d["pitch_bins"], (d["pitch_pred"] * d["pc"]).astype(f32))):
            want = torch.bucketize(torch.from_numpy(v), torch.from_numpy(bins), right=False).numpy()
            assert np.array_equal(sr.bucketize(bins, v), want)
            assert want[np.isnan(v)].tolist() == [255] * int(np.isnan(v).sum()) and np.isnan(v).any()
            assert np.all(np.diff(bins) > 0)


def test_duration_restatement_brackets_torch_and_the_float64_formula():
    import torch
    for log_d in (sc.dur_random(sc.DUR_SEEDS[0]), sc.dur_fences(), sc.dur_exact_inputs(130, "dur_scan_130")):
        ctl = np.full(log_d.shape, 0.75, f32)
        c = sr.duration_candidates(log_d, ctl)
        t = torch.from_numpy(log_d)
        tor = torch.clamp(torch.round(torch.exp(t) - 1) * 0.75, min=0).numpy()          # reference U/layers.py:218-221
        assert np.all((c == tor[None]).any(0))
        d64 = np.maximum(np.rint(np.exp(log_d.astype(np.float64)) - 1.0) * 0.75, 0.0)
        und = (sr.bits(c) != sr.bits(c[0])[None]).any(0)
        assert np.array_equal(c[sr.K_ULP][~und], d64[~und].astype(f32))
    assert np.array_equal(np.rint(np.array([0.5, 1.5, 2.5, -0.5], f32)), torch.round(torch.tensor([0.5, 1.5, 2.5, -0.5])).numpy())


def test_scan_and_frame_search_are_cumsum_and_searchsorted():
    r = sc.rng_of("scan_host")
    dur = r.choice([0.0, 0.5, 1.0, 2.75, 3.0], (3, 130)).astype(f32)
    cnt, cum, m64, m32 = sr.duration_scan(dur)
    assert np.array_equal(cnt, dur.astype(np.int64)) and np.array_equal(cum, np.cumsum(dur.astype(np.int64), 1)) and np.array_equal(m64, cum[:, -1])
    for L, T, H in sc.LR_CASES:
        d = sc.lr_data(L, T, H)
        ph = sr.frame_phoneme(d["cum"], T)
        for b in range(3):
            assert np.array_equal(ph[b], np.minimum(np.searchsorted(d["cum"][b], np.arange(T), side="right"), L - 1))
        for pos in (None, d["pos"]):
            y = sr.length_regulate_ref(d["x"], d["cum"], d["mel"], pos, T)
            want = np.take_along_axis(d["x"], ph[:, :, None], 1) * (np.arange(T)[None, :, None] < d["mel"][:, None, None])
            assert sr.same_bits(y, (want + (0 if pos is None else pos[None])).astype(f32))
        assert d["mel"][0] == 0 and d["mel"][1] == T and d["cum"][1, -1] < T


def test_f0_restatement_brackets_the_float64_coding():
    """f0_to_coarse (reference U/function.py:178-187) in float64 from the float32 products: where all candidates agree they give its bucket,
    except within a float32 rounding of a bucket edge (the float32 chain after the logarithm is part of the contract, not of K)."""
    for mode in (0, 1):
        d = sc.f0_random_case(mode, sc.F0_SEEDS[mode][0])
        f0, uvl = d["pitch_pred"][..., 0].astype(np.float64), d["pitch_pred"][..., 1]
        f0d = np.where(uvl > 0, 0.0, 2.0 ** f0 if mode == 1 else f0 * sc.F0_STD + sc.F0_MEAN)
        mel = 1127.0 * np.log(1.0 + f0d / 700.0)
        sc64 = np.where(mel > 0, (mel - sr.F0_MEL_MIN) * 254.0 / (sr.F0_MEL_MAX - sr.F0_MEL_MIN) + 1.0, mel)
        sc64 = np.clip(sc64, 1.0, 255.0)
        want = np.trunc(sc64 + 0.5).astype(np.int32)
        dec = sr.f0_decisions(d["pitch_pred"][..., 0], uvl, mode, sc.F0_MEAN, sc.F0_STD)
        far = np.abs(sc64 + 0.5 - np.rint(sc64 + 0.5)) > 1e-3
        assert np.array_equal(dec[dec.shape[0] // 2][far], want[far]) and far.mean() > 0.99
        assert want.min() < 30 and want.max() > 240 and np.any(want == 1)


def test_positions_are_torch_cumsum_times_mask():
    import torch
    for L, H in sc.VP_CASES:
        d = sc.vp_data(L, H)
        pos, y = sr.var_positions_ref(d["x"], d["table"], d["alpha"])
        m = torch.from_numpy(d["x"][..., 0]).ne(0).long()                               # reference U/function.py:28-38
        assert np.array_equal(pos, (torch.cumsum(m, 1) * m).numpy())
        t = torch.from_numpy(d["x"]) + torch.tensor(d["alpha"]) * torch.from_numpy(d["table"])[torch.from_numpy(pos).long()]   # U/layers.py:497-498
        assert sr.same_bits(y, t.numpy())
        if L >= 64:
            assert np.isnan(d["x"][0, :, 0]).any() and np.any(np.signbit(d["x"][0, :, 0]) & (d["x"][0, :, 0] == 0))
            assert pos[0].max() > 0 and pos[1].max() == 0 and pos[2, -1] == L


@pytest.mark.parametrize("nfft,hop,F", sc.ISTFT_CASES)
def test_istft_definition_is_torch_istft_and_the_share_at_pcm_boundaries_is_under_the_cap(nfft, hop, F):
    import torch
    q = sc.istft_data(nfft, hop, F)
    bins = nfft // 2 + 1
    ref = sr.istft_reference(q, nfft, hop)
    q64 = q.astype(np.float64)
    X = np.exp(q64[..., :bins]) * np.exp(1j * np.sin(q64[..., bins:]))
    want = torch.istft(torch.from_numpy(X).transpose(1, 2), nfft, hop, nfft, torch.hann_window(nfft, dtype=torch.float64), center=True).numpy()
    assert want.shape == ref["wav"].shape
    scale = np.abs(want).max()
    assert np.abs(ref["wav"] - want).max() <= 1e-12 * scale
    frames = np.fft.irfft(X, n=nfft, axis=-1)                                           # a third evaluation: numpy's inverse DFT, overlap-added
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)
    num, den = np.zeros((2, nfft + hop * (F - 1))), np.zeros(nfft + hop * (F - 1))
    for f in range(F):
        num[:, f * hop:f * hop + nfft] += frames[:, f] * win
        den[f * hop:f * hop + nfft] += win * win
    ola = (num / np.where(den > 0, den, 1.0))[:, nfft // 2:nfft // 2 + hop * (F - 1)]
    assert np.abs(ref["wav"] - ola).max() <= 1e-12 * scale
    r64 = sr.istft_eval(q, nfft, hop, np.float64)
    assert np.all(np.isfinite(ref["wav"])) and np.all(r64["den"] > 0.2) and np.abs(ref["wav"]).max() < 0.5
    # caps on the reference alone
    assert sr.pcm_boundary(ref["wav"], ref["bar"]).mean() <= 1e-3
    assert np.all(ref["dev"] <= 64 * ref["lin"]), "the float32 restatement itself is far outside the linear bar"
    # the restatement passes its own criterion
    got = dict(specphase=sr.istft_eval(q, nfft, hop, f32)["specphase"], wav=ref["wav32"], pcm=sr.pcm_of(ref["wav32"]))
    fails, fig = sr.check_istft(got, ref)
    assert not fails, fails


# ---------------------------------------------------------------- caps
def test_undecided_shares_of_the_seeded_inputs_are_under_the_cap():
    und = np.concatenate([sr.check_duration(sr.duration_ref(x, np.ones(x.shape, f32)), x, np.ones(x.shape, f32))[1].ravel()
                          for x in map(sc.dur_random, sc.DUR_SEEDS)])
    assert und.size >= 4000 and und.mean() <= 1e-3
    f0 = []
    for mode, seeds in sc.F0_SEEDS.items():
        for s in seeds:
            d = sc.f0_random_case(mode, s)
            fails, u = sr.check_variance_embed(_as_got(d, sr.variance_embed_ref(d)), d, ISENT)
            assert not fails, fails
            f0.append(u.ravel())
    f0 = np.concatenate(f0)
    assert f0.size >= 8000 and f0.mean() <= 1e-3
    # the fences do what they are for: some elements undecided, the outer neighbours decided
    assert 0 < sr.check_duration(sr.duration_ref(sc.dur_fences(), np.ones((3, 357), f32)), sc.dur_fences(), np.ones((3, 357), f32))[1].mean() < 0.9


# ---------------------------------------------------------------- mutations
def _as_got(d, r):
    """A restatement's outputs in the form the kernel leaves them: absent index arrays hold the sentinel."""
    full = np.full((d["B"], d["L"]), ISENT, np.int32)
    return dict(x=r["x"], pitch_pred=r["pitch_pred"], pitch_idx=full if r["pitch_idx"] is None else r["pitch_idx"],
                energy_idx=full if r["energy_idx"] is None else r["energy_idx"])


def _ve_fails(d, mut):
    if mut == "frame_largest":
        d2 = sc.finish(dict(d), mut)
        return sr.check_variance_embed(_as_got(d, sr.variance_embed_ref(d2)), d, ISENT)[0]
    return sr.check_variance_embed(_as_got(d, sr.variance_embed_ref(d, mut)), d, ISENT)[0]


VE_MUTATIONS = [
    ("le_search", lambda: sc.ve_sweep_case(1.0, 1.0)),
    ("ctl_after_bucket", lambda: sc.ve_sweep_case(0.75, 1.1)),
    ("uv_ge", sc.uv_case),
    ("flush_subnormal", sc.uv_case),
    ("wrong_feature_idx", lambda: sc.ve_geometry_case(2, 3, 4, 1, "scalar")),
    ("ee_first", lambda: sc.ve_geometry_case(2, 3, 256, 5, "utt")),
    ("frame_largest", lambda: sc.ve_frame_case(2, 6, 9, "phoneme")),
    ("plus_one_first", lambda: sc.f0_fence_case(0)),
    ("no_half", lambda: sc.f0_fence_case(0)),
    ("mode1_as_0", lambda: sc.f0_fence_case(1)),
]


@pytest.mark.parametrize("mut,case", VE_MUTATIONS, ids=[m for m, _ in VE_MUTATIONS])
def test_variance_embed_mutations_fail_the_criterion(mut, case):
    d = case()
    assert not _ve_fails(d, None)
    assert _ve_fails(d, mut), mut


def test_float32_mel_constants_move_no_decided_element():
    """mel_min / mel_range formed in float32 (1127.f * logf(1.f + 50.f / 700.f)): mel_min moves by 5e-5 (6 ulp), every bucket edge by
    1.3e-5 of a bucket.  One step of the float32 argument 1 + f0 / 700 is 3e-5 of a bucket or more, and K = 4 ulp of logf leave +-9e-6
    (lowest buckets) to +-3.5e-5 undecided around an edge: at the fences the mutant decides differently on dozens of elements, but on
    none that the candidates decide alike -- the decision tier cannot see this mutation at K = 4 (an exhaustive run over every float32
    prediction from 50 to 93 Hz in mode 0 found none either); the whole-model fixtures pin these constants (margins >= 1e-3)."""
    for mode in (0, 1):
        d = sc.f0_fence_case(mode)
        a, b = sr.variance_embed_ref(d)["pitch_idx"], sr.variance_embed_ref(d, "mel_consts32")["pitch_idx"]
        und = sr.check_variance_embed(_as_got(d, sr.variance_embed_ref(d)), d, ISENT)[1]
        assert (a != b).sum() >= 8 and np.all(und[a != b])
        assert not _ve_fails(d, "mel_consts32")


def test_every_variance_embed_case_passes_its_own_restatement():
    cases = [sc.ve_geometry_case(*c) for c in sc.VE_GEOMETRY] + [sc.ve_frame_case(*c) for c in sc.VE_FRAME] + [sc.uv_case(), sc.f0_fence_case(0), sc.f0_fence_case(1)]
    for d in cases:
        assert not _ve_fails(d, None), d["name"]
    d = sc.uv_case()
    r = sr.variance_embed_ref(d)
    assert r["pitch_pred"][1, 0, 1] == sc.SUBNORMAL and r["pitch_idx"][1, 0] == 1 and r["pitch_idx"][1, 1] > 1 and r["pitch_idx"][0, 1] > 1
    for mode in (0, 1):
        d = sc.f0_fence_case(mode)
        fails, und = sr.check_variance_embed(_as_got(d, sr.variance_embed_ref(d)), d, ISENT)
        e = sr.variance_embed_ref(d)["pitch_idx"].ravel()[d["n_edges"]:d["n_edges"] + d["n_ends"]]
        assert und.any() and e[0] == 1 and e[1] == 1 and 255 in e.tolist()
    for c in sc.VE_FRAME:     # the frame cases have zero-length phonemes and frames past the scan total
        d = sc.ve_frame_case(*c)
        assert np.any(np.diff(np.concatenate([np.zeros((3, 1), np.int32), d["cum"]], 1), axis=1) == 0) and (d["L"] == 1 or d["cum"][:, -1].min() < d["L"])


DUR_MUTATIONS = [   # (mutation, log_d, controls): the smallest case at which it shows
    ("no_carry", lambda: sc.dur_exact_inputs(65, "dur_scan_65"), 0.5),
    ("exclusive", lambda: np.array([[np.log(3.1)]] * 3, f32), 1.0),
    ("no_cap", lambda: np.array([[np.inf]] * 3, f32), 1.0),
    ("round_count", lambda: np.array([[np.log(2.1)]] * 3, f32), 1.5),      # dur 1.5: count 1, not 2
    ("clamp_first", lambda: np.array([[-np.inf]] * 3, f32), -2.0),         # (-1 * -2) = 2, not max(-1, 0) * -2
    ("trunc_round", lambda: sc.dur_fences(), 1.0),
    ("shift_one", lambda: sc.dur_fences(), 1.0),
]


@pytest.mark.parametrize("mut,make,ctl", DUR_MUTATIONS, ids=[m for m, _, _ in DUR_MUTATIONS])
def test_duration_mutations_fail_the_criterion(mut, make, ctl):
    log_d = make()
    c = np.full(log_d.shape, ctl, f32)
    assert not sr.check_duration(sr.duration_ref(log_d, c), log_d, c)[0]
    assert sr.check_duration(sr.duration_ref(log_d, c, mut), log_d, c)[0], mut


def test_round_half_up_differs_from_rint_only_at_exact_ties_which_no_k_decides():
    """floorf(e + 0.5f) against rintf(e): they differ only where e is exactly j + 0.5 with j even.  A candidate one ulp to either side of
    such an e decides for j and for j + 1, so the element is undecided for every K >= 1 and the rule of the decision tier cannot tell the
    two roundings apart; the mutations next to it (truncation, a shift by one) are caught at the fences."""
    log_d = sc.dur_fences()
    one = np.ones(log_d.shape, f32)
    a, b = sr.duration_candidates(log_d, one), sr.duration_candidates(log_d, one, mut="half_up")
    differ = (a != b)
    e = (sr.candidates(np.exp(log_d.astype(np.float64))) - f32(1.0)).astype(f32)
    assert differ.any() and np.all((e[differ] - np.floor(e[differ])) == 0.5)
    und1 = (sr.bits(sr.duration_candidates(log_d, one, k=1)) != sr.bits(sr.duration_candidates(log_d, one, k=1)[0])[None]).any(0)
    assert np.all(und1[differ[sr.K_ULP]])
    assert not sr.check_duration(sr.duration_ref(log_d, one, "half_up"), log_d, one)[0]


def test_duration_saturation_reference():
    L = 2112
    r = sr.duration_ref(np.full((3, L), np.inf, f32), np.ones((3, L), f32))
    assert r["cum"][0, 2046] == 2047 * 2 ** 20 and np.all(r["cum"][:, 2047:] == 2 ** 31 - 1)
    assert np.all(r["mel64"] == 2112 * 2 ** 20) and np.all(r["mel32"] == 2 ** 31 - 1)


def test_length_regulate_and_positions_mutations():
    L, T, H = 7, 40, 256
    d = sc.lr_data(L, T, H)
    assert not sr.same_bits(sr.length_regulate_ref(d["x"], d["cum"], d["mel"], None, T, mut="frame_largest"), sr.length_regulate_ref(d["x"], d["cum"], d["mel"], None, T))
    fma_seen = False
    for L, H in sc.VP_CASES:     # the fused form differs from the two roundings at the first case wide enough to hold such an element
        v = sc.vp_data(L, H)
        fma_seen = fma_seen or not sr.same_bits(sr.var_positions_ref(v["x"], v["table"], v["alpha"], mut="fma")[1], sr.var_positions_ref(v["x"], v["table"], v["alpha"])[1])
        if L == 64:
            assert fma_seen
            assert np.array_equal(sr.var_positions_ref(v["x"], v["table"], v["alpha"], mut="no_carry")[0], sr.var_positions_ref(v["x"], v["table"], v["alpha"])[0])
        if L == 65:
            assert not np.array_equal(sr.var_positions_ref(v["x"], v["table"], v["alpha"], mut="no_carry")[0], sr.var_positions_ref(v["x"], v["table"], v["alpha"])[0])


ISTFT_MUTATIONS = ("sym_hann", "drop_first_frame", "drop_last_frame", "nyquist_sign", "dc_doubled", "trim_off_by_one", "no_1_over_n")


@pytest.mark.parametrize("mut", ISTFT_MUTATIONS)
def test_istft_mutations_fail_the_criterion_at_the_smallest_case(mut):
    nfft, hop, F = (4, 1, 3) if mut != "sym_hann" else (4, 2, 5)
    q = sc.istft_data(nfft, hop, F)
    ref = sr.istft_reference(q, nfft, hop)
    m = sr.istft_eval(q, nfft, hop, f32, mut)
    fails, _ = sr.check_istft(dict(specphase=m["specphase"], wav=m["wav"], pcm=sr.pcm_of(m["wav"])), ref)
    assert any(f.startswith("wav") for f in fails), (mut, fails)


def test_rowdot_reference_masks_and_bars():
    x, w, b = np.ones((5, 4), f32), np.ones((2, 4), f32), np.array([0.5, -0.5], f32)
    out, bar = sr.rowdot_ref(x, w, b, [3], 5)
    assert out[:3].tolist() == [[4.5, 3.5]] * 3 and np.all(out[3:] == 0) and np.all(bar[3:] == 0) and np.all(bar[:3] > 0)
    assert sr.act_rows_ref([2 ** 24], 1, 2 ** 10, 2 ** 31 - 1).tolist() == [2 ** 31 - 1]
    assert sr.same_bits(sr.reflect_lrelu_ref(np.array([[[1.0] * 4, [-2.0] * 4]], f32), 0.01)[0, :, 0], np.array([-2.0, 1.0, -2.0], f32) * np.array([0.01, 1, 0.01], f32))


# ---------------------------------------------------------------- refusals (host only: a wrapper that refuses returns before it launches)
A = 0x10000          # a non-null, 16-byte aligned "pointer": never dereferenced on these paths


def _refusals():
    import small_harness as sh
    ve = dict(x=A, pitch_pred=A, energy_pred=A, p_control=1.0, e_control=1.0, f0_mean=0.0, f0_std=1.0, energy_bins=A, n_bins=256, pitch_emb=A,
              energy_emb=A, pitch_idx=A, energy_idx=A, B=1, L=2, H=4)
    return [
        ("embed null", lambda: sh.embed(None, A, A, A, 1, 1, 4, 2)),
        ("embed H % 4", lambda: sh.embed(A, A, A, A, 1, 1, 6, 2)),
        ("embed B", lambda: sh.embed(A, A, A, A, 0, 1, 4, 2)),
        ("embed L", lambda: sh.embed(A, A, A, A, 1, 0, 4, 2)),
        ("add_speaker null", lambda: sh.add_speaker(A, A, None, A, 1, 2, 1, 1, 4)),
        ("add_speaker ids", lambda: sh.add_speaker(A, A, A, A, 2, 2, 3, 1, 4)),
        ("add_speaker H % 4", lambda: sh.add_speaker(A, A, A, A, 1, 2, 1, 1, 6)),
        ("add_speaker rows", lambda: sh.add_speaker(A, A, A, A, 1, 2, 1, 0, 4)),
        ("var_positions null", lambda: sh.var_positions(A, None, A, 9, A, A, 1, 2, 4)),
        ("var_positions table", lambda: sh.var_positions(A, A, A, 2, A, A, 1, 2, 4)),
        ("var_positions H % 4", lambda: sh.var_positions(A, A, A, 9, A, A, 1, 2, 5)),
        ("rowdot null", lambda: sh.rowdot(A, A, None, A, None, 1, 1, 4, 1)),
        ("rowdot C % 4", lambda: sh.rowdot(A, A, A, A, None, 1, 1, 6, 1)),
        ("rowdot O = 0", lambda: sh.rowdot(A, A, A, A, None, 1, 1, 4, 0)),
        ("rowdot O = 3", lambda: sh.rowdot(A, A, A, A, None, 1, 1, 4, 3)),
        ("rowdot O = 4", lambda: sh.rowdot(A, A, A, A, None, 1, 1, 4, 4)),
        ("rowdot no rows", lambda: sh.rowdot(A, A, A, A, None, 0, 5, 4, 1)),
        ("rowdot x alignment", lambda: sh.rowdot(A + 4, A, A, A, None, 1, 1, 4, 1)),
        ("rowdot w alignment", lambda: sh.rowdot(A, A + 8, A, A, None, 1, 1, 4, 1)),
        ("duration null", lambda: sh.duration(A, 1.0, A, None, A, A, 1, 1)),
        ("duration dims", lambda: sh.duration(A, 1.0, A, A, A, A, 1, 0)),
        ("variance_embed null", lambda: sh.variance_embed(**{**ve, "energy_bins": None})),
        ("variance_embed feat", lambda: sh.variance_embed(**ve, feat=0)),
        ("variance_embed feat 4", lambda: sh.variance_embed(**ve, feat=4)),
        ("variance_embed mode", lambda: sh.variance_embed(**ve, pitch_mode=3)),
        ("variance_embed mode 2 without bins", lambda: sh.variance_embed(**ve, pitch_mode=2)),
        ("variance_embed n_bins", lambda: sh.variance_embed(**{**ve, "n_bins": 128})),
        ("variance_embed ctl N", lambda: sh.variance_embed(**ve, pctl=(A, 1, 0), N=3)),
        ("variance_embed ctl Lp", lambda: sh.variance_embed(**ve, ectl=(A, 1, 0), N=2, cum=A, Lp=0)),
        ("length_regulate null", lambda: sh.length_regulate(A, None, A, None, A, 1, 1, 1, 4)),
        ("length_regulate T", lambda: sh.length_regulate(A, A, A, None, A, 1, 1, 0, 4)),
        ("length_regulate H % 4", lambda: sh.length_regulate(A, A, A, None, A, 1, 1, 1, 3)),
        ("add_positions null", lambda: sh.add_positions(A, None, 1, 1, 4)),
        ("add_positions dims", lambda: sh.add_positions(A, A, 1, 0, 4)),
        ("add_positions H % 4", lambda: sh.add_positions(A, A, 1, 1, 2)),
        ("act_rows null", lambda: sh.act_rows(None, A, 1, 0, 1, 5)),
        ("act_rows B", lambda: sh.act_rows(A, A, 0, 0, 1, 5)),
        ("accum_div null", lambda: sh.accum_div(A, None, 4, 1.0)),
        ("accum_div n", lambda: sh.accum_div(A, A, 6, 1.0)),
        ("accum_div n = 0", lambda: sh.accum_div(A, A, 0, 1.0)),
        ("transpose null", lambda: sh.transpose_bct_btc(None, A, 1, 1, 1)),
        ("reflect_lrelu null", lambda: sh.reflect_lrelu(A, None, 1, 2, 4, 0.01)),
        ("reflect_lrelu n", lambda: sh.reflect_lrelu(A, A, 1, 1, 4, 0.01)),
        ("reflect_lrelu C % 4", lambda: sh.reflect_lrelu(A, A, 1, 2, 6, 0.01)),
        ("istft null", lambda: sh.istft(A, 18, None, A, A, A, 1, 2, 16, 4)),
        ("istft n_fft 2", lambda: sh.istft(A, 18, A, A, A, A, 1, 2, 2, 1)),
        ("istft n_fft 512", lambda: sh.istft(A, 514, A, A, A, A, 1, 2, 512, 128)),
        ("istft n_fft 24", lambda: sh.istft(A, 26, A, A, A, A, 1, 2, 24, 4)),
        ("istft hop 0", lambda: sh.istft(A, 18, A, A, A, A, 1, 2, 16, 0)),
        ("istft hop 3", lambda: sh.istft(A, 18, A, A, A, A, 1, 2, 16, 3)),
        ("istft hop = n_fft", lambda: sh.istft(A, 18, A, A, A, A, 1, 2, 16, 16)),
        ("istft hop = n_fft = 4", lambda: sh.istft(A, 6, A, A, A, A, 1, 3, 4, 4)),
        ("istft F", lambda: sh.istft(A, 18, A, A, A, A, 1, 1, 16, 4)),
        ("istft ldq", lambda: sh.istft(A, 17, A, A, A, A, 1, 2, 16, 4)),
        ("istft B", lambda: sh.istft(A, 18, A, A, A, A, 0, 2, 16, 4)),
    ]


def test_wrappers_refuse_bad_arguments_before_launching():
    import __graft_entry__ as g
    assert g.built_harness_small_hash() == g.harness_small_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    for name, call in _refusals():
        msg = call()
        assert isinstance(msg, str) and "launch failed" not in msg, (name, msg)


def test_hann_window_sum_vanishes_only_for_hop_equal_n_fft():
    """Why launch_istft refuses hop == n_fft and nothing else it admitted: the squared periodic Hann window overlap-added at hop is
    bounded away from 0 for every proper divisor hop of n_fft, and 0 at the frame joins for hop == n_fft (torch.istft refuses that pair)."""
    import torch
    for nfft in (4, 8, 16, 256):
        w2 = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)) ** 2
        for hop in [h for h in range(1, nfft + 1) if nfft % h == 0]:
            env = w2.reshape(nfft // hop, hop).sum(0)
            assert (env.min() > 0.2) == (hop < nfft), (nfft, hop, env.min())
    X = torch.ones(9, 3, dtype=torch.complex128)
    with pytest.raises(RuntimeError):
        torch.istft(X, 16, 16, 16, torch.hann_window(16, dtype=torch.float64), center=True)
