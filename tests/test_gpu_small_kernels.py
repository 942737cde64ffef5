"""Per-kernel tests (-m gpu) of the integer-decision and index kernels of csrc/small_kernels.hip: embedding, speaker add, predictor
positions, rowdot, duration rounding and scan, the f0 / energy buckets, the length regulator, act_rows, the join, the transpose and the
iSTFT tail, one launch wrapper at a time through tests/csrc/small_harness.hip (tests/small_harness.py), against the plain-numpy references
and criteria of tests/small_ref.py at the shapes and values of tests/small_cases.py.  The whole-model fixtures keep every discrete decision
away from its boundary; these tests put the inputs ON the boundaries.

Buffers follow tests/test_gpu_kernels.py: every device buffer is a view between NaN / -1 guard bands (Guarded), the one strided input
(the iSTFT's q) has NaN in its row gaps, outputs are pre-filled with a sentinel, bands and gaps must hold their bits afterwards, and "left
alone" means the sentinel survives.

Exact tier: bit for bit against the float32 restatement.  Decision tier (expf before the duration rounding; logf / powf before the f0
bucket): an element on which all 2 K + 1 candidates of the transcendental agree must match, any other must take one of their decisions
(small_ref.K_ULP = 4, assumed); the scan and the embedding rows are then restated from the kernel's own decisions.  Bars: rowdot and the
iSTFT (small_ref.istft_reference)."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import small_cases as sc   # noqa: E402
import small_ref as sr     # noqa: E402
from test_gpu_kernels import Guarded, i32, record   # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT = f32(-12345.5)
ISENT = -777
_T0 = time.time()
_undecided = {"duration": [0, 0], "f0": [0, 0]}     # [undecided, judged] over the seeded random elements of the module


@pytest.fixture(scope="module")
def sh():
    import torch
    assert torch.cuda.is_available(), "the kernel tests need the GPU"
    import small_harness
    import __graft_entry__ as g
    assert g.built_harness_small_hash() == g.harness_small_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    small_harness.load()
    assert g.harness_small_hash() in small_harness.version()
    return small_harness


def G(a):
    return Guarded(np.asarray(a))


def G64(a):
    """An int64 array as pairs of int32 (Guarded compares 2- and 4-byte elements): -1 bands, 16-byte aligned."""
    a = np.ascontiguousarray(a, np.int64)
    return Guarded(a.view(np.int32).reshape(-1))


def out_f(shape, sentinel=SENT):
    return Guarded(shape=shape, sentinel=sentinel)


def out_i(shape, dtype=np.int32, sentinel=ISENT):
    return Guarded(shape=shape, dtype=dtype, sentinel=dtype(sentinel))


def fetch(g, shape=None):
    body, ok = g.fetch()
    assert ok, "a guard band or a gap was written"
    return body.reshape(shape) if shape is not None else body


def fetch64(g, shape):
    return np.ascontiguousarray(fetch(g).reshape(-1)).view(np.int64).reshape(shape)


def unchanged(*gs):
    for g in gs:
        assert g is None or g.unchanged(), "an input buffer or its guard band was written"


def ptr(g):
    return None if g is None else g.ptr


# ---------------------------------------------------------------- embedding, speaker add
@pytest.mark.parametrize("B,L,H", sc.EMBED_CASES)
def test_embed(sh, B, L, H):
    """ids at -1, 0, n_rows - 1 and n_rows (the clamps) among random ones; one position row per l; H = 516: the block loop's second trip."""
    r = sc.rng_of(f"embed_{B}_{L}_{H}")
    n_rows = 11
    ids = r.integers(0, n_rows, (B, L))
    ids.ravel()[:4] = [-1, 0, n_rows - 1, n_rows][:ids.size]
    emb, pos = r.standard_normal((n_rows, H)).astype(f32), r.standard_normal((L, H)).astype(f32)
    gi, ge, gp, gx = G64(ids), G(emb), G(pos), out_f((B, L, H))
    assert sh.embed(gi.ptr, ge.ptr, gp.ptr, gx.ptr, B, L, H, n_rows) is None
    assert sr.same_bits(fetch(gx), sr.embed_ref(ids, emb, pos))
    unchanged(gi, ge, gp)


@pytest.mark.parametrize("n_ids", [1, 3])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("H", [4, 516])
def test_add_speaker(sh, n_ids, inplace, H):
    B, L, n_spk = 3, 5, 4
    r = sc.rng_of(f"spk_{n_ids}_{inplace}_{H}")
    xin, spk = r.standard_normal((B, L, H)).astype(f32), r.standard_normal((n_spk, H)).astype(f32)
    speaker = np.array([n_spk + 3] if n_ids == 1 else [-2, 1, n_spk], np.int64)     # out of range: clamped into the table
    gs, gk = G(spk), G64(speaker)
    gin = G(xin)
    gx = gin if inplace else out_f((B, L, H))
    assert sh.add_speaker(gin.ptr, gx.ptr, gs.ptr, gk.ptr, n_ids, n_spk, B, L, H) is None
    assert sr.same_bits(fetch(gx), sr.add_speaker_ref(xin, spk, speaker))
    unchanged(gs, gk, None if inplace else gin)


# ---------------------------------------------------------------- predictor positions
@pytest.mark.parametrize("L,H", sc.VP_CASES)
def test_var_positions(sh, L, H):
    """Positions across 64-lane chunks (-0.0 is zero; NaN and subnormals are not; an all-zero row; a row without zeros), table_rows = L + 1
    exactly, y = x + fl(alpha * table[pos]); then compute_positions = false on a second x reuses the first call's positions."""
    d = sc.vp_data(L, H)
    B = 3
    gx, gt, ga, gx2 = G(d["x"]), G(d["table"]), G(np.array([d["alpha"]] * 4, f32)), G(d["x2"])
    gpos, gy, gy2 = out_i((B, L)), out_f((B, L, H)), out_f((B, L, H))
    assert sh.var_positions(gx.ptr, gpos.ptr, gt.ptr, L + 1, ga.ptr, gy.ptr, B, L, H, True) is None
    pos, y = sr.var_positions_ref(d["x"], d["table"], d["alpha"])
    assert np.array_equal(fetch(gpos, (B, L)), pos)
    assert sr.same_bits(fetch(gy), y)
    assert pos[1].max() == 0 and pos[2, -1] == L
    assert sh.var_positions(gx2.ptr, gpos.ptr, gt.ptr, L + 1, ga.ptr, gy2.ptr, B, L, H, False) is None
    assert np.array_equal(fetch(gpos, (B, L)), pos)
    assert sr.same_bits(fetch(gy2), sr.var_positions_ref(d["x2"], d["table"], d["alpha"], posbuf=pos)[1])
    unchanged(gx, gt, ga, gx2)


# ---------------------------------------------------------------- rowdot
@pytest.mark.parametrize("C,O,with_lens", sc.ROWDOT_CASES)
def test_rowdot(sh, C, O, with_lens):
    """B * L = 5 rows (not a multiple of the 4 rows of a block); C = 260 / 1028: lanes with one float4 more than their neighbours; with
    lens the last two rows are masked and must be exactly 0."""
    r = sc.rng_of(f"rowdot_{C}_{O}_{with_lens}")
    B, L = 1, 5
    x, w, b = r.standard_normal((B * L, C)).astype(f32), r.standard_normal((O, C)).astype(f32), r.standard_normal(O).astype(f32)
    lens = [3] if with_lens else None
    gx, gw, gb, go = G(x), G(w), G(b), out_f((B * L, O))
    gl = i32(lens) if with_lens else None
    assert sh.rowdot(gx.ptr, gw.ptr, gb.ptr, go.ptr, gl.data_ptr() if with_lens else None, B, L, C, O) is None
    got = fetch(go, (B * L, O))
    ref, bar = sr.rowdot_ref(x, w, b, lens, L)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err[bar == 0] == 0) and np.all(got[bar == 0] == 0)
    ratio = float((err[bar > 0] / bar[bar > 0]).max())
    print(f"[rowdot] C {C} O {O} lens {with_lens}: worst err / bar {ratio:.3g}")
    record("rowdot", C=C, O=O, lens=with_lens, ratio=ratio)
    assert ratio <= 1.0
    unchanged(gx, gw, gb)


# ---------------------------------------------------------------- duration
def run_duration(sh, log_d, values=None, strides=(0, 0), scalar=1.0):
    B, L = log_d.shape
    gl = G(log_d)
    gv = G(values) if values is not None else None
    gd, gc, g64, g32 = out_f((B, L)), out_i((B, L)), out_i((2 * B,)), out_i((B,))
    assert sh.duration(gl.ptr, scalar, gd.ptr, gc.ptr, g64.ptr, g32.ptr, B, L, ctl=(ptr(gv), strides[0], strides[1])) is None
    got = dict(dur=fetch(gd, (B, L)), cum=fetch(gc, (B, L)), mel64=fetch64(g64, (B,)), mel32=fetch(g32, (B,)))
    unchanged(gl, gv)
    return got


@pytest.mark.parametrize("L", sc.DUR_SCAN_L)
@pytest.mark.parametrize("form", sc.CTL_FORMS)
def test_duration_scan_and_dyadic_controls(sh, L, form):
    """Inclusive scan across 64-lane chunks, B = 3 independent rows (one all zero), dyadic controls against integer rint values (dur
    fractional, the repeat count its truncation), in the three CtlRef forms; the forms agree where they describe the same controls."""
    log_d = sc.dur_exact_inputs(L, f"dur_scan_{L}")
    values, strides, scalar = sc.ctl_values(form, 3, L, sc.rng_of(f"dur_ctl_{L}_{form}"))
    ctl = sc.ctl_of(values, strides, scalar, 3, L)
    got = run_duration(sh, log_d, values, strides, scalar)
    fails, und = sr.check_duration(got, log_d, ctl)
    assert not fails, fails
    assert not und.any(), "the exact cases are decided for every candidate"
    assert np.any(got["dur"] != np.trunc(got["dur"])) or L == 1
    if form == "scalar":   # the same controls as arrays
        for v, s in ((np.full(3, scalar, f32), (1, 0)), (np.full(3 * L, scalar, f32), (L, 1))):
            again = run_duration(sh, log_d, v, s, 7.0)
            assert all(np.array_equal(got[k], again[k]) for k in got)


def test_duration_clamp_infinities_and_nan(sh):
    """e = 0 (log_d = 0) and e = -1 (log_d = -inf) under controls of either sign: the clamp at 0 after the control; +inf: dur inf, the
    count capped at 2^20; NaN (log_d or control, and inf * 0): count 0 and dur 0 (csrc/kernels.h)."""
    log_d = np.array([[0.0, 0.0, -np.inf, -np.inf, np.inf, np.nan, np.log(3.0), np.inf, np.log(3.0)]] * 3, f32)
    ctl = np.array([[2.0, -2.0, 2.0, -2.0, 1.0, 1.0, np.nan, 0.0, -1.5]] * 3, f32)
    ctl[1] *= f32(0.5)
    got = run_duration(sh, log_d, ctl.ravel(), (log_d.shape[1], 1), 7.0)
    fails, und = sr.check_duration(got, log_d, ctl)
    assert not fails and not und.any(), fails
    assert got["dur"][0].tolist() == [0.0, 0.0, 0.0, 2.0, np.inf, 0.0, 0.0, 0.0, 0.0]
    assert got["cum"][0].tolist() == [0, 0, 0, 2, 2 + 2 ** 20, 2 + 2 ** 20, 2 + 2 ** 20, 2 + 2 ** 20, 2 + 2 ** 20]
    assert got["cum"][1, 3] == 1 and got["mel64"][0] == 2 + 2 ** 20


def test_duration_saturation(sh):
    """L = 2112, all +inf: 2^20 frames per phoneme; cum saturates at 2^31 - 1 from the 2048th phoneme on, mel64 = 2112 * 2^20 exactly,
    mel32 saturated."""
    L = 2112
    log_d = np.full((3, L), np.inf, f32)
    got = run_duration(sh, log_d)
    fails, _ = sr.check_duration(got, log_d, np.ones((3, L), f32))
    assert not fails, fails
    assert np.all(np.isinf(got["dur"]))
    assert got["cum"][0, 2046] == 2047 * 2 ** 20 and np.all(got["cum"][:, 2047:] == 2 ** 31 - 1)
    assert np.all(got["mel64"] == 2112 * 2 ** 20) and np.all(got["mel32"] == 2 ** 31 - 1)


@pytest.mark.parametrize("seed", sc.DUR_SEEDS + ("fences",))
def test_duration_decisions(sh, seed):
    """rint(expf(log_d) - 1): seeded log_d in [-2, 3.5], and the fences log(j + 1.5) with their neighbours out to +-8 ulp."""
    log_d = sc.dur_fences() if seed == "fences" else sc.dur_random(seed)
    B, L = log_d.shape
    got = run_duration(sh, log_d)
    fails, und = sr.check_duration(got, log_d, np.ones((B, L), f32))
    print(f"[duration] {seed}: {int(und.sum())} of {und.size} elements undecided at K = {sr.K_ULP}")
    record("duration", seed=seed, undecided=int(und.sum()), elements=int(und.size))
    if seed != "fences":
        _undecided["duration"][0] += int(und.sum())
        _undecided["duration"][1] += und.size
    else:
        assert und.any() and not und.all()
    assert not fails, fails


# ---------------------------------------------------------------- variance_embed
def run_ve(sh, d):
    B, L, H, mode = d["B"], d["L"], d["H"], d["mode"]
    gx, gpp, gep = G(d["x"]), G(d["pitch_pred"]), G(d["energy_pred"])
    geb, gpb, gpe, gee = G(d["energy_bins"]), G(d["pitch_bins"]), G(d["pitch_emb"]), G(d["energy_emb"])
    gpi, gei = out_i((B, L)), out_i((B, L))
    gpv = G(d["p_values"]) if d["p_values"] is not None else None
    gev = G(d["e_values"]) if d["e_values"] is not None else None
    gcum = G(d["cum"]) if d["cum"] is not None else None
    msg = sh.variance_embed(gx.ptr, gpp.ptr, gep.ptr, d["p_scalar"], d["e_scalar"], d["f0_mean"], d["f0_std"], geb.ptr, sr.N_BINS, gpe.ptr, gee.ptr,
                            gpi.ptr, gei.ptr, B, L, H, pitch_mode=mode, pitch_bins=gpb.ptr, feat=d["feat"],
                            pctl=(ptr(gpv),) + tuple(d["p_strides"]), ectl=(ptr(gev),) + tuple(d["e_strides"]), N=L, cum=ptr(gcum), Lp=d["Lp"])
    assert msg is None, msg
    got = dict(x=fetch(gx), pitch_pred=fetch(gpp, d["pitch_pred"].shape), pitch_idx=fetch(gpi, (B, L)), energy_idx=fetch(gei, (B, L)))
    unchanged(gep, geb, gpb, gpe, gee, gpv, gev, gcum)
    return got


def judge_ve(sh, d):
    got = run_ve(sh, d)
    fails, und = sr.check_variance_embed(got, d, ISENT)
    assert not fails, (d["name"], fails)
    return got, und


@pytest.mark.parametrize("pc,ec", [(1.0, 1.0), (0.75, 1.1)])
def test_buckets_at_every_boundary(sh, pc, ec):
    """Mode 2 pitch and energy: predictions whose product with the control is bins[k] or a float32 neighbour, for every k; below the first
    and above the last bin; +-inf; NaN (index 255, as torch.bucketize).  Dyadic and non-dyadic scalar controls; pitch_pred keeps its bits."""
    d = sc.ve_sweep_case(pc, ec)
    got, _ = judge_ve(sh, d)
    nan = np.isnan(d["energy_pred"])
    assert nan.any() and np.all(got["energy_idx"][nan] == 255) and np.all(got["pitch_idx"][np.isnan(d["pitch_pred"])] == 255)
    assert got["energy_idx"].min() == 0 and got["energy_idx"].max() == 255 and got["pitch_idx"].min() == 0


@pytest.mark.parametrize("mode,feat,H,L,form", sc.VE_GEOMETRY)
def test_variance_embed_geometry(sh, mode, feat, H, L, form):
    """feat 1 / 2 / 3 (the absent feature's index array keeps its sentinel, one add or two), H up to the block loop's second trip, the
    three CtlRef forms, the three pitch modes."""
    judge_ve(sh, sc.ve_geometry_case(mode, feat, H, L, form))


@pytest.mark.parametrize("mode,Lp,N,form", sc.VE_FRAME)
def test_variance_embed_frame_level_controls(sh, mode, Lp, N, form):
    """Controls per phoneme, rows per frame: scans with zero-length phonemes at the front, in the middle and at the end; frames at and
    past the utterance's last frame take phoneme Lp - 1."""
    judge_ve(sh, sc.ve_frame_case(mode, Lp, N, form))


def test_uv_rule_at_the_signed_zeros_and_subnormals(sh):
    d = sc.uv_case()
    got, und = judge_ve(sh, d)
    assert not und.any()
    uv = got["pitch_pred"][..., 1]
    assert uv[1, 0] == sc.SUBNORMAL and uv[1, 1] == -sc.SUBNORMAL, "the product that underflows to a subnormal must not be flushed"
    assert got["pitch_idx"].tolist() == [[got["pitch_idx"][0, 0]] * 2, [1, got["pitch_idx"][1, 1]], [1, got["pitch_idx"][2, 1]]]
    assert got["pitch_idx"][0, 0] > 1 and got["pitch_idx"][1, 1] > 1 and got["pitch_idx"][2, 1] > 1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", [0, 1, "fences"])
def test_f0_bucket_decisions(sh, mode, which):
    """Modes 0 / 1 (logf; powf and logf): seeded f0 over 40 .. 1200 Hz; a dozen bucket edges with neighbours out to +-8 ulp and the exact
    ends of the coding (f0d <= 0, log(0), uv, huge, inf: decided; NaN: any index inside the table)."""
    d = sc.f0_fence_case(mode) if which == "fences" else sc.f0_random_case(mode, sc.F0_SEEDS[mode][which])
    got, und = judge_ve(sh, d)
    print(f"[f0] mode {mode} {d['name']}: {int(und.sum())} of {und.size} elements undecided at K = {sr.K_ULP}")
    record("f0", mode=mode, case=d["name"], undecided=int(und.sum()), elements=int(und.size))
    if which == "fences":
        assert und.any()
        ends = got["pitch_idx"].ravel()[d["n_edges"]:d["n_edges"] + d["n_ends"]]
        assert np.all((ends >= 0) & (ends <= 255))
        assert ends.tolist()[:2] == [1, 1]
    else:
        _undecided["f0"][0] += int(und.sum())
        _undecided["f0"][1] += und.size


# ---------------------------------------------------------------- length regulator, add_positions
@pytest.mark.parametrize("L,T,H", sc.LR_CASES)
@pytest.mark.parametrize("with_pos", [False, True])
def test_length_regulate(sh, L, T, H, with_pos):
    d = sc.lr_data(L, T, H)
    gx, gc, gm, gp, gy = G(d["x"]), G(d["cum"]), G(d["mel"]), G(d["pos"]) if with_pos else None, out_f((3, T, H))
    assert sh.length_regulate(gx.ptr, gc.ptr, gm.ptr, ptr(gp), gy.ptr, 3, L, T, H) is None
    assert sr.same_bits(fetch(gy), sr.length_regulate_ref(d["x"], d["cum"], d["mel"], d["pos"] if with_pos else None, T))
    unchanged(gx, gc, gm, gp)


@pytest.mark.parametrize("L,T,H", sc.LR_CASES)
def test_add_positions(sh, L, T, H):
    d = sc.lr_data(L, T, H)
    y = sc.rng_of(f"addpos_{T}_{H}").standard_normal((3, T, H)).astype(f32)
    gy, gp = G(y), G(d["pos"])
    assert sh.add_positions(gy.ptr, gp.ptr, 3, T, H) is None
    assert sr.same_bits(fetch(gy), (y + d["pos"][None]).astype(f32))
    unchanged(gp)


# ---------------------------------------------------------------- act_rows, accum_div, transpose, reflect_lrelu
@pytest.mark.parametrize("B", sc.ACT_ROWS_B)
def test_act_rows(sh, B):
    """cap hit and not hit in one launch, add_rows, and (lens + add) * mul beyond int32 before the cap."""
    r = sc.rng_of(f"act_rows_{B}")
    lens = r.integers(0, 2 ** 24, B).astype(np.int32)
    lens[0] = 3
    for add, mul, cap, add_rows in ((2, 256, 10 ** 6, 0), (0, 256, 2 ** 31 - 1, 5), (1, 2 ** 10, 2 ** 31 - 1, 0), (0, 1, 2 ** 30, 123)):
        gl, go = G(lens), out_i((B,))
        assert sh.act_rows(gl.ptr, go.ptr, B, add, mul, cap, add_rows) is None
        want = sr.act_rows_ref(lens, add, mul, cap, add_rows)
        assert np.array_equal(fetch(go, (B,)), want)
        unchanged(gl)
    assert B == 1 or (np.any(want < 2 ** 30) and int(((lens.astype(np.int64) + 1) * 2 ** 10).max()) > 2 ** 31)


@pytest.mark.parametrize("n,with_k,div", sc.ACCUM_CASES)
def test_accum_div(sh, n, with_k, div):
    r = sc.rng_of(f"accum_{n}_{with_k}_{div}")
    S, Sj, Sk = (r.standard_normal(n).astype(f32) for _ in range(3))
    gS, gj, gk = G(S), G(Sj), G(Sk) if with_k else None
    assert sh.accum_div(gS.ptr, gj.ptr, n, div, Sk=ptr(gk)) is None
    assert sr.same_bits(fetch(gS, (n,)), sr.accum_div_ref(S, Sj, Sk if with_k else None, div))
    unchanged(gj, gk)


@pytest.mark.parametrize("C", sc.TRANSPOSE_CT)
@pytest.mark.parametrize("T", sc.TRANSPOSE_CT)
def test_transpose(sh, C, T):
    x = sc.rng_of(f"tr_{C}_{T}").standard_normal((2, C, T)).astype(f32)
    gx, go = G(x), out_f((2, T, C))
    assert sh.transpose_bct_btc(gx.ptr, go.ptr, 2, C, T) is None
    assert sr.same_bits(fetch(go), x.transpose(0, 2, 1))
    unchanged(gx)


@pytest.mark.parametrize("n,C", sc.REFLECT_CASES)
def test_reflect_lrelu(sh, n, C):
    x = sc.rng_of(f"reflect_{n}_{C}").standard_normal((2, n, C)).astype(f32)
    gx, go = G(x), out_f((2, n + 1, C))
    assert sh.reflect_lrelu(gx.ptr, go.ptr, 2, n, C, 0.01) is None
    assert sr.same_bits(fetch(go), sr.reflect_lrelu_ref(x, 0.01))
    unchanged(gx)


# ---------------------------------------------------------------- iSTFT
@pytest.mark.parametrize("nfft,hop,F", sc.ISTFT_CASES)
def test_istft(sh, nfft, hop, F):
    """wav + pcm on a dense q, wav only on a q with 6 NaN columns per row, pcm only: specphase within K ulp, wav inside the bar per
    sample, pcm the conversion of the kernel's own wav and equal to the reference's off the rounding boundaries."""
    B, bins, nsamp = 2, nfft // 2 + 1, hop * (F - 1)
    ref = sr.istft_reference(sc.istft_data(nfft, hop, F), nfft, hop)
    for pad, want_wav, want_pcm in ((0, True, True), (6, True, False), (0, False, True)):
        q = sc.istft_data(nfft, hop, F, pad)
        gq = Guarded(q[..., :2 * bins], ld=2 * bins + pad)
        gsp, gri = out_f((B, F, 2 * bins)), out_f((B, F, 2 * bins))
        gw = out_f((B, nsamp)) if want_wav else None
        gp = out_i((B, nsamp), np.int16, -31111) if want_pcm else None
        assert sh.istft(gq.ptr, 2 * bins + pad, gsp.ptr, gri.ptr, ptr(gw), ptr(gp), B, F, nfft, hop) is None
        got = dict(specphase=fetch(gsp), wav=fetch(gw, (B, nsamp)) if want_wav else None, pcm=fetch(gp, (B, nsamp)) if want_pcm else None)
        fetch(gri)
        unchanged(gq)
        fails, fig = sr.check_istft(got, ref)
        print(f"[istft] n_fft {nfft} hop {hop} F {F} pad {pad}: {fig}, float32 restatement's worst deviation / linear bar "
              f"{float((ref['dev'] / ref['lin']).max()):.3g}")
        record("istft", nfft=nfft, hop=hop, F=F, pad=pad, **fig)
        assert not fails, fails


def test_undecided_shares_and_wall_time():
    """The seeded random elements the kernel left undecided stay under the cap the CPU test asserts on the reference alone (1e-3, pooled
    per family); the module's wall time is recorded."""
    for fam, (u, n) in _undecided.items():
        print(f"[{fam}] undecided {u} of {n} seeded elements")
        record(fam, pooled_undecided=u, pooled_elements=int(n))
        assert u <= 1e-3 * n
    record("small_wall", seconds=time.time() - _T0)
    print(f"[small kernels] wall time {time.time() - _T0:.1f} s")
