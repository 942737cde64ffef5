"""The pitch library's kernels against the float64 definition (tests/f0_ref.py), split where a discrete decision is taken: the
autocorrelation per element under its derived bar; the candidates on the frames whose every decision has a margin above that bar; the path
search alone on the reference's own candidates (deterministic: the path is equal in every frame); then the whole forward, and the targets
against models.f0_targets on the GPU's own track.  The cases and their reference are built once (tests/f0_cases.py)."""
import numpy as np
import pytest

import f0_cases as fc
import f0_ref as fr
from e2e_tts_amd import config as cfgmod, f0 as f0lib
from e2e_tts_amd.models import f0_targets

pytestmark = pytest.mark.gpu

_C, _T = {}, {}


def case(name):
    if name not in _C:
        c = fc.build(name)
        _C[name] = (c, fc.reference(c))
    return _C[name]


def tracker(sr, hop):
    if (sr, hop) not in _T:
        _T[sr, hop] = f0lib.PitchTracker(sr, hop)
    return _T[sr, hop]


def wide(wavs):
    """The same rows in an array with audio_stride > n"""
    buf = np.full((wavs.shape[0], wavs.shape[1] + 37), 9, wavs.dtype)
    buf[:, :wavs.shape[1]] = wavs
    return buf[:, :wavs.shape[1]]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_autocorrelation_per_element(name):
    c, refs = case(name)
    t = tracker(c["sr"], c["hop"])
    t.poison_workspace()
    r = t.debug_acf(wide(c["wavs"]), c["n_valid"])
    worst, worst_abs = 0.0, 0.0
    for b, ref in enumerate(refs):
        T = ref["T"]
        assert not r[b, T:].any()                                                  # frames >= T_b are written as 0
        err = np.abs(r[b, :T].astype(np.float64) - ref["r"])
        v = ref["valid"]
        assert not r[b, :T][~v].any()                                              # r_a[0] == 0: r = 0 throughout
        if v.any():
            worst = max(worst, float((err[v] / ref["bar_r"][v]).max()))
            worst_abs = max(worst_abs, float(err[v].max()))
    print(f"{name}: max |r - r64| = {worst_abs:.3e}, worst err / bar = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(fc.CASES))
def test_candidates_on_decided_frames(name):
    c, refs = case(name)
    t = tracker(c["sr"], c["hop"])
    t.poison_workspace()
    f, s = t.debug_candidates(wide(c["wavs"]), c["n_valid"])
    K = t.K
    compared = worst_f = worst_s = 0
    for b, ref in enumerate(refs):
        T = ref["T"]
        assert not f[b, T:].any() and not s[b, T:].any()
        for k in range(T):
            gf, gs = f[b, k].astype(np.float64), s[b, k].astype(np.float64)
            assert gf[0] == 0 and np.isfinite(gs[0])
            held = gs[1:] > -np.inf
            assert not (np.diff(held.astype(np.int8)) > 0).any()                    # the empty slots are the last ones
            assert (gf[1:][~held] == 0).all() and (gf[1:][held] > 0).all()
            assert (np.diff(gs[1:][held]) <= 0).all()                               # descending strength
            assert abs(gs[0] - ref["strength"][k, 0]) <= ref["bar_s"][k, 0] + 2 * fr.U * abs(gs[0])
            if not ref["frame_ok"][k]:
                continue
            compared += 1
            want = ref["strength"][k, 1:] > -np.inf
            assert held.sum() == want.sum(), (b, k)
            lag_ref = ref["lag"][k, 1:][want]
            lag_got = np.rint(c["sr"] / gf[1:][held]).astype(np.int64)            # |d| <= 1/2: the lag is the nearest integer, up to a tie
            order_ref, order_got = np.argsort(lag_ref), np.argsort(gf[1:][held])[::-1]
            rf, rs_, bf, bs = (ref[q][k, 1:][want][order_ref] for q in ("freq", "strength", "bar_f", "bar_s"))
            assert (np.abs(lag_got[order_got] - lag_ref[order_ref]) <= 1).all(), (b, k)
            ef, es = np.abs(gf[1:][held][order_got] - rf) / bf, np.abs(gs[1:][held][order_got] - rs_) / bs
            worst_f, worst_s = max(worst_f, float(ef.max(initial=0))), max(worst_s, float(es.max(initial=0)))
    print(f"{name}: {compared} frames compared, worst |f - f64| / bar = {worst_f:.4f}, worst |s - s64| / bar = {worst_s:.4f}")
    assert compared >= 0.95 * sum(r["T"] for r in refs)
    assert worst_f <= 1.0 and worst_s <= 1.0


@pytest.mark.parametrize("name", list(fc.CASES))
def test_path_on_the_references_candidates(name):
    c, refs = case(name)
    t = tracker(c["sr"], c["hop"])
    T = max(r["T"] for r in refs)
    f, s = np.zeros((len(refs), T, t.K), np.float32), np.zeros((len(refs), T, t.K), np.float32)
    for b, r in enumerate(refs):
        f[b, :r["T"]], s[b, :r["T"]] = r["freq"], r["strength"]
    frames = np.array([r["T"] for r in refs], np.int32)
    t.poison_workspace()
    got = t.debug_path(f, s, frames)
    for b, r in enumerate(refs):
        want, _, margin = fr.viterbi(f[b, :r["T"]], s[b, :r["T"]], c["sr"], c["hop"])   # on the rounded candidates: what the kernel was given
        assert margin >= fc.MIN_PATH_MARGIN
        assert np.array_equal(got[b, :r["T"]], want.astype(np.float32)), b
        assert not got[b, r["T"]:].any()


def test_path_ties_go_to_the_lower_index():
    t = tracker(22050, 256)
    K, T = t.K, 6
    f, s = np.zeros((2, T, K), np.float32), np.full((2, T, K), -np.inf, np.float32)
    # row 0: candidates 1 and 2 are the same voiced candidate twice, stronger than the unvoiced one: every predecessor and the end tie
    f[0, :, 1:3], s[0, :, 1:3], s[0, :, 0] = 200.0, 0.9, 0.5
    # row 1: the unvoiced candidate and a voiced one tie at the end of a one-frame path, and frames beyond `frames` are not read
    f[1, 0, 1], s[1, 0, 0], s[1, 0, 1] = 300.0, 0.75, 0.75
    f[1, 1:], s[1, 1:] = np.nan, np.nan
    got = t.debug_path(f, s, np.array([T, 1], np.int32))
    assert np.array_equal(got[0], np.full(T, 200.0, np.float32))
    assert got[1, 0] == 0 and not got[1, 1:].any()
    # the same through the reference, which reports the ties as zero margins
    want, idx, margin = fr.viterbi(f[0], s[0], 22050, 256)
    assert (idx == 1).all() and margin == 0.0 and np.array_equal(want, got[0])
    # a tie between DIFFERENT voiced predecessors of one cell: frame 0 holds two candidates an octave either side of frame 1's
    f2, s2 = np.zeros((1, 2, K), np.float32), np.full((1, 2, K), -np.inf, np.float32)
    f2[0, 0, 1], f2[0, 0, 2], f2[0, 1, 1] = 100.0, 400.0, 200.0
    s2[0, :, 0], s2[0, 0, 1], s2[0, 0, 2], s2[0, 1, 1] = 0.1, 0.8, 0.8, 0.9
    got2 = t.debug_path(f2, s2, np.array([2], np.int32))
    assert got2[0, 0] == 100.0 and got2[0, 1] == 200.0


@pytest.mark.parametrize("name", list(fc.CASES))
def test_forward_end_to_end(name):
    c, refs = case(name)
    t = tracker(c["sr"], c["hop"])
    t.poison_workspace()
    r = t.forward(wide(c["wavs"]), c["n_valid"])
    f0 = r["f0"]
    assert np.array_equal(r["lens"], c["n_valid"] // c["hop"]) and r["T"] == f0.shape[1]
    compared = 0
    for b, ref in enumerate(refs):
        T = ref["T"]
        assert not f0[b, T:].any()
        t.poison_workspace()
        one = t.forward(c["wavs"][b:b + 1, :max(int(c["n_valid"][b]), 1)], c["n_valid"][b:b + 1])["f0"]
        assert np.array_equal(one[0, :T], f0[b, :T]), b                                # row b is bit-identical to its B = 1 call
        if not (T and fc.compared(ref)):
            continue
        compared += 1
        assert np.array_equal(f0[b, :T] == 0, ref["f0"] == 0), b
        bar = ref["bar_f"][np.arange(T), ref["index"]]
        assert (np.abs(f0[b, :T].astype(np.float64) - ref["f0"]) <= bar + fr.U * ref["f0"]).all(), b
    assert compared >= 1


@pytest.mark.parametrize("name", ["mixed_22k", "edges_16k"])
def test_targets_on_the_gpus_own_track(name):
    c, _ = case(name)
    t = tracker(c["sr"], c["hop"])
    t.poison_workspace()
    r = t.forward(c["wavs"], c["n_valid"])
    track, lens = r["f0"], r["lens"]
    stats = cfgmod.DEFAULT_STATS
    lin_f0, lin_uv = t.targets(stats)
    log_f0, log_uv = t.targets(None, "log", 1e-9)
    for b, T in enumerate(lens):
        T = int(T)
        want_f0, want_uv = f0_targets(track[b, :T].astype(np.float64), stats)
        assert np.array_equal(lin_f0[b, :T], want_f0.astype(np.float32)) and np.array_equal(lin_uv[b, :T], want_uv), b
        assert not lin_f0[b, T:].any() and not lin_uv[b, T:].any() and not log_f0[b, T:].any() and not log_uv[b, T:].any()
        wl, wu = f0_targets(track[b, :T].astype(np.float64), stats, "log", 1e-9)
        wl = wl.astype(np.float32)
        assert np.array_equal(log_uv[b, :T], wu)
        assert (np.abs(log_f0[b, :T] - wl) <= np.spacing(np.abs(wl))).all(), b           # 1 fp32 ulp
    # the all-zero row of edges_16k is an all-unvoiced row
    if name == "edges_16k":
        assert not track[2].any() and not lin_f0[2].any() and (lin_uv[2, :int(lens[2])] == 1).all()


def test_targets_single_voiced_frame_and_all_unvoiced():
    """Tracks made by the path kernel from constructed candidates: one voiced frame in the middle, none at all, voiced ends only."""
    t = tracker(22050, 256)
    K, T = t.K, 300                                     # more frames than the targets kernel has threads: chunks of two
    f, s = np.zeros((3, T, K), np.float32), np.full((3, T, K), -np.inf, np.float32)
    s[:, :, 0] = 0.5
    f[0, 150, 1], s[0, 150, 1] = 180.0, 5.0
    for k in (0, 1, 2, 297, 299):
        f[2, k, 1], s[2, k, 1] = 100.0 + k, 5.0
    frames = np.array([T, T - 7, T], np.int32)
    track = t.debug_path(f, s, frames)
    assert (track[0] != 0).sum() == 1 and not track[1].any() and (track[2] != 0).sum() == 5
    stats = cfgmod.DEFAULT_STATS
    for mode in ("linear", "log"):
        got_f0, got_uv = t.targets(stats, mode, 1e-9)
        for b in range(3):
            n = int(frames[b])
            want_f0, want_uv = f0_targets(track[b, :n].astype(np.float64), stats, mode, 1e-9)
            want_f0 = want_f0.astype(np.float32)
            assert np.array_equal(got_uv[b, :n], want_uv) and not got_f0[b, n:].any() and not got_uv[b, n:].any()
            if mode == "linear":
                assert np.array_equal(got_f0[b, :n], want_f0), b
            else:
                assert (np.abs(got_f0[b, :n] - want_f0) <= np.spacing(np.abs(want_f0))).all(), b
        assert not got_f0[1].any()                                                     # an all-unvoiced row becomes 0
        assert (got_f0[0, :int(frames[0])] == got_f0[0, 150]).all()                    # one voiced frame: constant
