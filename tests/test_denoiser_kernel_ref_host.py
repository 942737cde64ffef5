"""CPU checks of what tests/test_gpu_denoiser_kernels.py relies on (tests/denoiser_kernel_ref.py, tests/denoiser_kernel_cases.py):
  - the restatements against independent evaluations (torch's reflect pad, torch float32 arithmetic as the reference writes it,
    denoiser_ref.envelope, explicit PCM values);
  - that the cases reach what they are for (exact zeros, the FLT_MIN rule, the frame clamp, every special bin);
  - mutations: a fused mag - bias * strength differs at every strength whose product is inexact and provably cannot at strength 0; a
    dropped frame clamp, an off-by-one reflection and a rounding PCM conversion each differ;
  - every refusal of the seven launch wrappers (they return before launching, so this needs no GPU)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoiser_kernel_cases as dc   # noqa: E402
import denoiser_kernel_ref as dr     # noqa: E402
import denoiser_ref                  # noqa: E402

f32 = np.float32


# ---------------------------------------------------------------- restatements against independent evaluations
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_pad_refs_against_torch(N, hop):
    import torch
    half = N // 2
    c = dc.pad_case(N, hop)
    out = dr.stft_pad_ref(c["wav"], c["n_valid"], c["R"], N, hop)
    assert not np.isnan(out).any() and not out[0].any()
    for b, nb in enumerate(c["n_valid"]):
        if nb > half:
            t = torch.nn.functional.pad(torch.from_numpy(c["wav"][b, :nb])[None, None], (half, half), mode="reflect")[0, 0].numpy()
            assert dr.diff_count(out[b, :nb + N], t) == 0 and not out[b, nb + N:].any()
    assert (c["n_valid"][2] + N) % 4 != 0 and c["R"] * hop > max(c["n_valid"]) + N + hop
    for left, right in dc.EDGES:
        s = dc.stream_pad_case(N, hop, left, right)
        o = dr.stft_pad_stream_ref(s["seg"], s["L"], N, hop, left, right)
        t = torch.nn.functional.pad(torch.from_numpy(s["seg"])[None], (half if left else 0, half if right else 0), mode="reflect")[0].numpy()
        assert dr.diff_count(o, t) == 0 and o.shape[1] == s["Rq"] * hop


@pytest.mark.parametrize("strength", dc.STRENGTHS)
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_subtract_ref_against_torch_and_the_model_restatement(N, hop, strength):
    """The reference's own lines in torch float32 -- re^2 + im^2, clamp(mag - bias * strength, 0) -- give the restatement's sum of squares
    and md bit for bit on the finite bins; the root is checked against the float64 root rounded once more (innocuous for a square root:
    53 >= 2 * 24 + 2), because torch's vectorised CPU sqrt is not correctly rounded (one ulp off on 1 of 129 bins of the (256, 32) case);
    denoiser_ref._subtract (the whole-model restatement) gives the restatement's output."""
    import torch
    c = dc.spec_case(N, hop, strength)
    bins = c["bins"]
    row = c["spec"][1, 0]
    re, im, mag, md = dr.subtract_row_ref(row[:bins], row[bins:2 * bins], c["bias"], strength)
    tre, tim, tb = (torch.from_numpy(np.ascontiguousarray(a)) for a in (row[:bins], row[bins:2 * bins], c["bias"]))
    tsq = (tre ** 2 + tim ** 2).numpy()
    fin = np.isfinite(mag)
    with np.errstate(all="ignore"):
        assert dr.diff_count(mag[fin], np.sqrt(tsq.astype(np.float64)).astype(f32)[fin]) == 0
    tmd = torch.clamp(torch.from_numpy(mag) - tb * strength, min=0.0)
    assert dr.diff_count(md[fin], tmd.numpy()[fin]) == 0
    plain = c["spec"][2, :c["frames"][2]]                      # an utterance without special bins
    with np.errstate(all="ignore"):
        m = denoiser_ref._subtract(plain[:, :2 * bins], c["bias"], strength, bins)
    got = dr.spectral_subtract_ref(c["spec"], c["bias"], c["frames"], N, c["nov"], strength)[2, :c["frames"][2]]
    assert dr.diff_count(got[:, :2 * bins], m) == 0 and not got[:, 2 * bins:].any()


def test_special_bins_do_what_they_are_for():
    c = dc.spec_case(64, 32, 0.1)
    bins = c["bins"]
    row = c["spec"][1, 0]
    re, im, mag, md = dr.subtract_row_ref(row[:bins], row[bins:2 * bins], c["bias"], 0.1)
    assert md[3] == 0 and re[3] == 0 and mag[3] > 0                              # bias above the magnitude
    assert mag[4] == c["bias"][4] * f32(0.1) and md[4] == 0 and not np.signbit(md[4])
    assert mag[5] == 0 and np.signbit(re[5]) and not np.signbit(im[5])           # -0 * 0 = -0
    assert mag[6] == f32(1.5)
    assert mag[7] == 0 and row[7] != 0 and re[7] == 0 and np.signbit(im[7])       # squares underflow: sc = 0
    assert 0 < mag[8] < 2e-20 and 0 < row[8] * row[8] < dr.FLT_MIN               # the root of a subnormal
    assert np.isnan(re[9]) and np.isnan(im[9])                                  # inf: sc = inf / inf
    assert np.isnan(mag[10]) and md[10] == 0 and re[10] == 0 and np.isnan(im[10])   # NaN: fmax(NaN, 0) = 0, NaN > 0 is false, sc = 0
    assert mag[11] == 0
    assert c["frames"] == [1, c["R"] - c["nov"] + 1, 5]


@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_ola_ref_against_the_envelope_and_the_cases_reach_their_paths(N, hop):
    for holes in (False, True):
        c = dc.ola_case(N, hop, holes)
        half, win, F = N // 2, c["win_sq"], c["frames"][0]
        env = denoiser_ref.envelope(win, F, hop)
        mine = np.array([dr.env_at(win, p, F, hop) for p in range(len(env))], f32)
        assert dr.diff_count(mine, env) == 0
        want = dr.ola_norm_ref(c["y"], c["inp"], c["n_valid"], c["frames"], win, c["n"], N, hop)
        nb = c["n_valid"][0]
        ola = c["y"][0, :len(env)].copy()
        keep = ~np.isnan(ola)
        with np.errstate(all="ignore"):
            ok = env > dr.FLT_MIN
            ola[ok] = ola[ok] / env[ok]
            ola *= f32(N / hop)
        assert dr.diff_count(want[0, :nb][keep[half:half + nb]], ola[half:half + nb][keep[half:half + nb]]) == 0
        assert dr.diff_count(want[2, :24], c["inp"][2, :24]) == 0 and not want[2, 24:].any() and not want[1, c["n_valid"][1]:].any()
        assert bool(np.any((env[half:half + nb] > 0) & (env[half:half + nb] <= dr.FLT_MIN))) == holes and bool(np.any(env[half:half + nb] == 0)) == holes
        # the frame clamp binds in the row's last samples wherever half > hop: without it the envelope there differs
        assert any(dr.env_at(win, p, F, hop) != dr.env_at(win, p, F + 8, hop) for p in range(nb, nb + half)) == (N // hop > 2)


def test_pcm_rails():
    assert dr.pcm_ref((dc.PCM_RAILS / 32768).astype(f32)).tolist() == dc.PCM_RAILS_WANT
    assert dr.pcm_ref(np.array([0.99999, -0.99999, 2.9e-5, -2.9e-5, np.inf, -np.inf], f32)).tolist() == [32767, -32767, 0, 0, 32767, -32768]


# ---------------------------------------------------------------- mutations
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_a_fused_subtraction_differs_except_at_an_exact_product(N, hop):
    """mag - bias * strength as one fma changes output elements at strengths 0.1, 0.75 and 10 at every geometry; at strength 0 the product is
    exactly 0 whatever its rounding, so the mutation provably cannot show there."""
    for s in dc.STRENGTHS:
        c = dc.spec_case(N, hop, s)
        a = dr.spectral_subtract_ref(c["spec"], c["bias"], c["frames"], N, c["nov"], s)
        b = dr.spectral_subtract_ref(c["spec"], c["bias"], c["frames"], N, c["nov"], s, contract=True)
        nd = dr.diff_count(a, b)
        print(f"[contract] ({N}, {hop}) strength {s:g}: {nd} of {a.size} elements")
        assert (nd == 0) if s == 0 else (nd > 0), (s, nd)


def test_other_mutations_differ():
    N, hop = 128, 32
    c = dc.pad_case(N, hop)
    want = dr.stft_pad_ref(c["wav"], c["n_valid"], c["R"], N, hop)
    nb = c["n_valid"][2]
    bad = want.copy()
    bad[2, nb + N // 2:nb + N] = c["wav"][2, :nb][::-1][:N // 2]         # the edge sample repeated (a 'symmetric' pad)
    assert dr.diff_count(bad, want) > 0
    o = dc.ola_case(N, hop)
    w = dr.ola_norm_ref(o["y"], o["inp"], o["n_valid"], o["frames"], o["win_sq"], o["n"], N, hop)
    unclamped = dr.ola_norm_ref(o["y"], o["inp"], o["n_valid"], [f + 8 for f in o["frames"]], o["win_sq"], o["n"], N, hop)
    assert dr.diff_count(unclamped[:2], w[:2]) > 0
    with np.errstate(all="ignore"):
        rounded = np.clip(np.nan_to_num(np.rint(w * f32(32768)), nan=-32768), -32768, 32767).astype(np.int16)
    assert dr.diff_count(rounded, dr.pcm_ref(w)) > 0


# ---------------------------------------------------------------- refusals (host only: a wrapper that refuses returns before it launches)
A = 0x10000          # a non-null, 16-byte aligned "pointer": never dereferenced on these paths


def _refusals():
    import denoiser_harness as dh
    MAXLL = dh.LLONG_MAX
    return [
        ("stft_pad null wav", lambda: dh.stft_pad(None, 8, A, A, 1, 4, 64, 32)),
        ("stft_pad null n_valid", lambda: dh.stft_pad(A, 8, None, A, 1, 4, 64, 32)),
        ("stft_pad null out", lambda: dh.stft_pad(A, 8, A, None, 1, 4, 64, 32)),
        ("stft_pad n_overlap 3", lambda: dh.stft_pad(A, 8, A, A, 1, 4, 96, 32)),
        ("stft_pad hop % 32", lambda: dh.stft_pad(A, 8, A, A, 1, 4, 64, 16)),
        ("stft_pad hop > 1024", lambda: dh.stft_pad(A, 8, A, A, 1, 4, 4096, 2048)),
        ("stft_pad B 0", lambda: dh.stft_pad(A, 8, A, A, 0, 4, 64, 32)),
        ("stft_pad B 65536", lambda: dh.stft_pad(A, 8, A, A, 65536, 4, 64, 32)),
        ("stft_pad R 0", lambda: dh.stft_pad(A, 8, A, A, 1, 0, 64, 32)),
        ("stft_pad wav_bs < 0", lambda: dh.stft_pad(A, -1, A, A, 1, 4, 64, 32)),
        ("stft_pad out unaligned", lambda: dh.stft_pad(A, 8, A, A + 4, 1, 4, 64, 32)),
        ("spectral_subtract null spec", lambda: dh.spectral_subtract(None, A, A, 1, 4, 96, 64, 2, 0.1)),
        ("spectral_subtract null bias", lambda: dh.spectral_subtract(A, None, A, 1, 4, 96, 64, 2, 0.1)),
        ("spectral_subtract null frames", lambda: dh.spectral_subtract(A, A, None, 1, 4, 96, 64, 2, 0.1)),
        ("spectral_subtract B 0", lambda: dh.spectral_subtract(A, A, A, 0, 4, 96, 64, 2, 0.1)),
        ("spectral_subtract B 65536", lambda: dh.spectral_subtract(A, A, A, 65536, 4, 96, 64, 2, 0.1)),
        ("spectral_subtract R 0", lambda: dh.spectral_subtract(A, A, A, 1, 0, 96, 64, 2, 0.1)),
        ("spectral_subtract filter_length odd", lambda: dh.spectral_subtract(A, A, A, 1, 4, 96, 63, 2, 0.1)),
        ("spectral_subtract filter_length 0", lambda: dh.spectral_subtract(A, A, A, 1, 4, 96, 0, 2, 0.1)),
        ("spectral_subtract Cpad % 4", lambda: dh.spectral_subtract(A, A, A, 1, 4, 98, 64, 2, 0.1)),
        ("spectral_subtract Cpad < 2 bins", lambda: dh.spectral_subtract(A, A, A, 1, 4, 64, 64, 2, 0.1)),
        ("spectral_subtract Cpad > 16384", lambda: dh.spectral_subtract(A, A, A, 1, 4, 16388, 64, 2, 0.1)),
        ("spectral_subtract spec unaligned", lambda: dh.spectral_subtract(A + 4, A, A, 1, 4, 96, 64, 2, 0.1)),
        ("spectral_subtract n_overlap 0", lambda: dh.spectral_subtract(A, A, A, 1, 4, 96, 64, 0, 0.1)),
        ("spectral_subtract n_overlap 3", lambda: dh.spectral_subtract(A, A, A, 1, 4, 96, 64, 3, 0.1)),
        ("spectral_subtract n_overlap 16", lambda: dh.spectral_subtract(A, A, A, 1, 4, 96, 64, 16, 0.1)),
        ("bias_frame null row", lambda: dh.bias_frame(None, A, 64)),
        ("bias_frame null bias", lambda: dh.bias_frame(A, None, 64)),
        ("bias_frame filter_length 0", lambda: dh.bias_frame(A, A, 0)),
        ("bias_frame filter_length odd", lambda: dh.bias_frame(A, A, 63)),
        ("ola_norm null y", lambda: dh.ola_norm(None, A, 8, A, A, A, A, A, 1, 8, 4, 64, 32)),
        ("ola_norm null in", lambda: dh.ola_norm(A, None, 8, A, A, A, A, A, 1, 8, 4, 64, 32)),
        ("ola_norm null n_valid", lambda: dh.ola_norm(A, A, 8, None, A, A, A, A, 1, 8, 4, 64, 32)),
        ("ola_norm null frames", lambda: dh.ola_norm(A, A, 8, A, None, A, A, A, 1, 8, 4, 64, 32)),
        ("ola_norm null win_sq", lambda: dh.ola_norm(A, A, 8, A, A, None, A, A, 1, 8, 4, 64, 32)),
        ("ola_norm no output", lambda: dh.ola_norm(A, A, 8, A, A, A, None, None, 1, 8, 4, 64, 32)),
        ("ola_norm geometry", lambda: dh.ola_norm(A, A, 8, A, A, A, A, A, 1, 8, 4, 64, 64)),
        ("ola_norm B 0", lambda: dh.ola_norm(A, A, 8, A, A, A, A, A, 0, 8, 4, 64, 32)),
        ("ola_norm n 0", lambda: dh.ola_norm(A, A, 8, A, A, A, A, A, 1, 0, 4, 64, 32)),
        ("ola_norm R 0", lambda: dh.ola_norm(A, A, 8, A, A, A, A, A, 1, 8, 0, 64, 32)),
        ("ola_norm in_bs < 0", lambda: dh.ola_norm(A, A, -1, A, A, A, A, A, 1, 8, 4, 64, 32)),
        ("ola_norm grid", lambda: dh.ola_norm(A, A, 8, A, A, A, A, A, 1, 2 ** 41, 4, 64, 32)),
        ("stft_pad_stream null seg", lambda: dh.stft_pad_stream(None, 64, A, 1, 64, 2, 64, 32, False, False)),
        ("stft_pad_stream null out", lambda: dh.stft_pad_stream(A, 64, None, 1, 64, 2, 64, 32, False, False)),
        ("stft_pad_stream geometry", lambda: dh.stft_pad_stream(A, 64, A, 1, 64, 2, 64, 48, False, False)),
        ("stft_pad_stream B 0", lambda: dh.stft_pad_stream(A, 64, A, 0, 64, 2, 64, 32, False, False)),
        ("stft_pad_stream L 0", lambda: dh.stft_pad_stream(A, 64, A, 1, 0, 2, 64, 32, False, False)),
        ("stft_pad_stream Rq 0", lambda: dh.stft_pad_stream(A, 64, A, 1, 64, 0, 64, 32, False, False)),
        ("stft_pad_stream seg_bs < L", lambda: dh.stft_pad_stream(A, 63, A, 1, 64, 2, 64, 32, False, False)),
        ("stft_pad_stream real edge, L == half", lambda: dh.stft_pad_stream(A, 64, A, 1, 32, 2, 64, 32, True, False)),
        ("stft_pad_stream L = half + 1 (off the hop grid)", lambda: dh.stft_pad_stream(A, 64, A, 1, 33, 3, 64, 32, True, True)),
        ("stft_pad_stream rows do not match", lambda: dh.stft_pad_stream(A, 64, A, 1, 64, 3, 64, 32, False, False)),
        ("stft_pad_stream out unaligned", lambda: dh.stft_pad_stream(A, 64, A + 8, 1, 64, 2, 64, 32, False, False)),
        ("fill_i32 null", lambda: dh.fill_i32(None, 4, 1)),
        ("fill_i32 n 0", lambda: dh.fill_i32(A, 0, 1)),
        ("ola_norm_stream null in", lambda: dh.ola_norm_stream(A, 64, 0, None, 8, A, A, A, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream null win_sq", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, None, A, A, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream no output", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, None, None, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream null y, not pass", lambda: dh.ola_norm_stream(None, 64, 0, A, 8, A, A, A, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream geometry", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 1, 8, 0, 1, 64, 24, False)),
        ("ola_norm_stream B 0", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 0, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream n 0", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 1, 0, 0, 1, 64, 32, False)),
        ("ola_norm_stream in_bs < n", lambda: dh.ola_norm_stream(A, 64, 0, A, 7, A, A, A, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream p_abs0 < 0", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 1, 8, -1, 1, 64, 32, False)),
        ("ola_norm_stream F_abs 0", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 1, 8, 0, 0, 64, 32, False)),
        ("ola_norm_stream y_off < 0", lambda: dh.ola_norm_stream(A, 64, -1, A, 8, A, A, A, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream range past y", lambda: dh.ola_norm_stream(A, 64, 60, A, 8, A, A, A, 1, 8, 0, 1, 64, 32, False)),
        ("ola_norm_stream position overflow", lambda: dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 1, 8, MAXLL - 7, 1, 64, 32, False)),
        ("ola_norm_stream position overflow, pass", lambda: dh.ola_norm_stream(None, 0, 0, A, 8, A, A, A, 1, 8, MAXLL - 7, 1, 64, 32, True)),
    ]


def test_wrappers_refuse_bad_arguments_before_launching():
    import __graft_entry__ as g
    assert g.built_harness_denoiser_hash() == g.harness_denoiser_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    import denoiser_harness as dh
    assert g.harness_denoiser_hash() in dh.version()
    for name, call in _refusals():
        msg = call()
        assert isinstance(msg, str) and "launch failed" not in msg, (name, msg)
    # the refusals added with these tests name their reason
    assert "n_overlap" in dh.spectral_subtract(A, A, A, 1, 4, 96, 64, 3, 0.1)
    assert "overflows" in dh.ola_norm_stream(A, 64, 0, A, 8, A, A, A, 1, 8, dh.LLONG_MAX - 7, 1, 64, 32, False)
