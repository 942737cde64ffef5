"""GPU tests (-m gpu) of the teacher-forced acoustic pass (e2etts_acoustic_forced, csrc/teacher.hip, UnsupervisedFastSpeech2.forward)
against the fixtures the reference's own forward generated (tools/make_forced_goldens.py), at the fixtures' shapes.

Bars: durations, mel lengths, bucket indices and uv exact; the targets at the model's level within twice the module's own
fp32-vs-float64 distance; dec_in / mel / mel_post on valid rows mean-L1 < 1e-4 (the project's HIP bar); the soft expansion per element
against the float64 product by the bars of tests/kernel_ref.py for a chain of K = txt_len fp32 terms (gamma_n S per element, 4 x a
float32 evaluation's RMS in aggregate)."""
import numpy as np
import pytest

import forced_cases as fc
import kernel_ref as kr
from conftest import load_golden, states_for

pytestmark = pytest.mark.gpu

HIP_BAR = 1e-4
WANT = ("dur", "mel_lens", "pitch_idx", "energy_idx", "log_d", "pitch_pred", "energy_pred")
_ENG = {}


def engine_of(g):
    from e2e_tts_amd.runtime import engine_from_states
    key = (str(g["variant"]), int(g["weight_seed"]))
    if key not in _ENG:
        cfg, ac, voc = fc.states_of(g, vocoder=True)
        _ENG[key] = engine_from_states(cfg, fc.STATS, ac, voc, device=0)
    return fc.states_of(g)[0], _ENG[key]


def run_forced(eng, g, si, precision="fp32", want=WANT, **over):
    """The fixture's step si (0: soft expansion, 1: length regulator) through the engine, targets frame-resolved as the reference takes them."""
    eng.set_precision("fp32", precision)
    p_t, e_t = fc.targets_of(g)
    kw = dict(durations=g[f"s{si}_dur"], T=int(g["attn_soft"].shape[1]), pitch_frames=True, energy_frames=True, p_control=float(g["p_control"]))
    if si == 0:
        kw.update(attn_soft=g["attn_soft"], mel_lens=g["mel_lens"])
    if isinstance(p_t, dict):
        kw.update(f0=p_t["f0"], uv=p_t["uv"])
    elif p_t is not None:
        kw.update(pitch=p_t)
    if e_t is not None:
        kw.update(energy=e_t)
    kw.update(over)
    r = eng.acoustic_forced(g["ids"], g["txt_lens"], g["speakers"], want=want, **kw)
    mel, mel_post = eng.fetch_mel(r["B"], r["T"])
    return r, mel, mel_post


def check_fixture(eng, cfg, g, si, r, mel, mel_post, float_bar=HIP_BAR, taps=True):
    pre = f"s{si}_"
    B, L = g["ids"].shape
    T = r["T"]
    ve = cfg["models"]["fastspeech2"]["variance"]["variance_embedding"]
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    pf, ef = ve["pitch_feature"] == "frame_level", ve["energy_feature"] == "frame_level"
    out_lens = g[pre + "mel_lens"]
    assert T == g["attn_soft"].shape[1]
    np.testing.assert_array_equal(r["dur"], g[pre + "dur"])
    np.testing.assert_array_equal(r["mel_lens"], out_lens)
    # indices: every row of a phoneme_level feature the fixture holds; valid frames of a frame_level one in soft mode (the map's padded rows
    # are the caller's), every frame in hard mode
    for name, frame in (("pitch_idx", pf), ("energy_idx", ef)):
        for b in range(B):
            n = int(out_lens[b]) if frame else L
            np.testing.assert_array_equal(r[name][b, :n], g[pre + name][b, :n], err_msg=f"{name} row {b}")
    stride = int(g["row_stride"])
    figs = {}
    if taps:
        if pre + "p_f0" in g:
            t = eng.fetch_tap("pitch_target", (B, T if pf else L, 2))
            rows = out_lens if pf else g["txt_lens"]
            figs["p_f0"] = fc.valid_mean_l1(t[..., 0], g[pre + "p_f0"], rows)
            assert figs["p_f0"] <= 2.0 * float(g[pre + "p_f0_err"]), figs
            for b, n in enumerate(rows):
                np.testing.assert_array_equal(t[b, :n, 1], g[pre + "p_uv"][b, :n])
        if pre + "p_pitch" in g:
            t = eng.fetch_tap("pitch_target", (B, T if pf else L))
            figs["p_pitch"] = fc.valid_mean_l1(t, g[pre + "p_pitch"], out_lens if pf else g["txt_lens"])
            assert figs["p_pitch"] <= 2.0 * float(g[pre + "p_pitch_err"]), figs
        if pre + "e_tgt" in g:
            t = eng.fetch_tap("energy_target", (B, T if ef else L))
            figs["e_tgt"] = fc.valid_mean_l1(t, g[pre + "e_tgt"], out_lens if ef else g["txt_lens"])
            assert figs["e_tgt"] <= 2.0 * float(g[pre + "e_tgt_err"]), figs
        figs["dec_in"] = fc.valid_mean_l1(eng.fetch_tap("dec_in", (B, T, H)), g[pre + "dec_in"], out_lens, stride)
    figs["mel"] = fc.valid_mean_l1(mel, g[pre + "mel"], out_lens, stride)
    figs["mel_post"] = fc.valid_mean_l1(mel_post, g[pre + "mel_post"], out_lens, stride)
    print(f"[forced] step {si}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k in ("dec_in", "mel", "mel_post"):
        if k in figs:
            assert figs[k] < float_bar, figs
    return figs


@pytest.mark.parametrize("si", [0, 1], ids=["soft", "hard"])
@pytest.mark.parametrize("name", fc.MODEL_FIXTURES)
def test_fixture_fp32(name, si):
    """Every fixture, both steps, exact fp32: discrete outputs exact, targets as the reference embeds them, dec_in / mel / mel_post on valid rows."""
    g = fc.load(name)
    cfg, eng = engine_of(g)
    r, mel, mel_post = run_forced(eng, g, si)
    check_fixture(eng, cfg, g, si, r, mel, mel_post)
    # the predictors still run: their outputs are returned (before the control where the feature has a target)
    ve = cfg["models"]["fastspeech2"]["variance"]["variance_embedding"]
    assert fc.valid_mean_l1(r["log_d"], g[f"s{si}_log_d"], g["txt_lens"]) < fc.bar(g, f"s{si}_log_d")
    for k, feat in (("pitch_pred", "pitch_feature"), ("energy_pred", "energy_feature")):
        rows = g[f"s{si}_mel_lens"] if ve[feat] == "frame_level" else g["txt_lens"]
        assert r[k].shape == g[f"s{si}_{k}"].shape
        assert fc.valid_mean_l1(r[k], g[f"s{si}_{k}"], rows) < fc.bar(g, f"s{si}_{k}"), k


@pytest.mark.parametrize("name", ["forced_tiny_b3", "forced_full_b2"])
def test_fixture_bf16x3_decoder(name):
    """Split-precision decoder: the discrete decisions lie upstream of it and stay exact; mel_post within the same bar."""
    g = fc.load(name)
    cfg, eng = engine_of(g)
    try:
        for si in (0, 1):
            r, mel, mel_post = run_forced(eng, g, si, precision="bf16x3")
            check_fixture(eng, cfg, g, si, r, mel, mel_post, taps=False)
    finally:
        eng.set_precision("fp32", "fp32")


SOFT_SHAPES = [(70, 12, 64), (33, 7, 64), (5, 1, 64), (150, 70, 64), (300, 40, 384)]   # one partial row tile; K below one k-step; K across chunks; H across column tiles


@pytest.mark.parametrize("T,K,H", SOFT_SHAPES)
def test_soft_expansion_per_element(T, K, H):
    """launch_soft_expand alone, on guarded buffers: an utterance of K phonemes inside a map padded to L = K + 3 columns whose padding
    (map and phoneme rows) is NaN -- it must not be read --, next to a full-length one; every element against the float64 product."""
    from test_gpu_kernels import Guarded, i32
    lib = fc.harness()
    import __graft_entry__ as ge
    assert ge.built_harness_forced_hash() == ge.harness_forced_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    rng = kr.rng_of(f"soft_expand_{T}_{K}_{H}")
    L = K + 3
    lens = [K, L]
    B = 2
    attn = rng.random((B, T, L)).astype(np.float32)
    attn /= attn.sum(-1, keepdims=True)
    x = rng.standard_normal((B, L, H)).astype(np.float32)
    pos = rng.standard_normal((T, H)).astype(np.float32)
    attn[0, :, K:] = np.nan
    x[0, K:] = np.nan
    ga, gx, gp = Guarded(attn), Guarded(x), Guarded(pos)
    out = Guarded(shape=(B, T, H), sentinel=np.float32(-12345.5))
    msg = lib.e2ekt_soft_expand(ga.ptr, gx.ptr, i32(lens).data_ptr(), None, None, gp.ptr, out.ptr, B, T, L, H, None)
    assert msg is None, msg
    got, guard_ok = out.fetch()
    assert guard_ok and ga.unchanged() and gx.unchanged() and gp.unchanged()
    for b, n in enumerate(lens):
        a64, x64 = attn[b, :, :n].astype(np.float64), x[b, :n].astype(np.float64)
        ref = a64 @ x64 + pos
        S = np.abs(a64) @ np.abs(x64) + np.abs(pos)
        err = np.abs(got[b].astype(np.float64) - ref)
        assert np.all(np.isfinite(got[b]))
        elem = float((err / (kr.gamma(n + 1) * S)).max())
        # the float32 yardstick: the same chain blocked in K by 32
        y = np.zeros((T, H), np.float32)
        for k0 in range(0, n, 32):
            y = (y + attn[b, :, k0:min(n, k0 + 32)] @ x[b, k0:min(n, k0 + 32)]).astype(np.float32)
        y = (y + pos).astype(np.float32)
        ys, gs = kr.rel_rms(np.abs(y.astype(np.float64) - ref), S), kr.rel_rms(err, S)
        print(f"[soft_expand] T {T} K {n} H {H}: worst err / bar {elem:.3g}, rms {gs:.3g} (float32 numpy {ys:.3g})")
        assert elem <= 1.0
        if err.size >= kr.AGG_MIN_ELEMS:
            assert gs <= kr.AGG_FACTOR * ys if ys > 0 else gs == 0


def test_frame2phoneme_kernel_matches_the_reference_function():
    """launch_teacher_scan on the direct fixture: zero durations before, between and after (the in-place quirk), phonemes of more than 8
    and more than 128 frames (numpy's summation paths): means and uv marks equal the reference function's bit for bit; cum and mel lengths are the scan."""
    import ctypes as C
    import torch
    lib = fc.harness()
    g = fc.load("forced_frame2phoneme")
    dur, lens = g["dur"], g["lens"]
    B, L = dur.shape
    T = g["frames"].shape[1]
    d = torch.from_numpy(dur.copy()).cuda()
    tl = torch.from_numpy(lens.astype(np.int32)).cuda()
    cum = torch.full((B, L), -7, dtype=torch.int32, device="cuda")
    m64 = torch.zeros(B, dtype=torch.int64, device="cuda")
    m32 = torch.zeros(B, dtype=torch.int32, device="cuda")
    src = [torch.from_numpy(g["frames"]).cuda(), torch.from_numpy(g["uv"]).cuda(), torch.from_numpy(g["uv"]).cuda()]
    dst = [torch.full((B, L), float("nan"), device="cuda") for _ in range(3)]
    srcs = (C.c_void_p * 3)(*[t.data_ptr() for t in src])
    dsts = (C.c_void_p * 3)(*[t.data_ptr() for t in dst])
    uvs = (C.c_int * 3)(0, 0, 1)
    msg = lib.e2ekt_teacher_scan(d.data_ptr(), tl.data_ptr(), cum.data_ptr(), m64.data_ptr(), m32.data_ptr(), None, 3, srcs, dsts, uvs, B, L, T, None)
    assert msg is None, msg
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy(), dur)
    np.testing.assert_array_equal(cum.cpu().numpy(), np.cumsum(dur.astype(np.int64), 1))
    np.testing.assert_array_equal(m64.cpu().numpy(), dur.astype(np.int64).sum(1))
    np.testing.assert_array_equal(m32.cpu().numpy(), dur.astype(np.int64).sum(1))
    np.testing.assert_array_equal(dst[0].cpu().numpy().view(np.uint32), g["means"].view(np.uint32))
    np.testing.assert_array_equal(dst[1].cpu().numpy().view(np.uint32), g["uv_means"].view(np.uint32))
    np.testing.assert_array_equal(dst[2].cpu().numpy(), np.where(g["uv_means"] == 1.0, 1.0, 0.0).astype(np.float32))


def test_device_durations_are_clamped_as_the_header_says():
    """launch_teacher_scan on durations that lie in device memory and were never validated: NaN and negative values count as 0, a
    fraction is truncated, a value above 2^20 (inf included) counts as 2^20, every slot at or past the utterance's length counts as 0;
    the clamped values are written back, cum / mel lengths / means are those of the clamped durations (the restatement on them, bit for
    bit), and given mel lengths (soft mode) are clamped to [0, T]."""
    import ctypes as C
    import torch
    import forced_ref as fr
    lib = fc.harness()
    rng = kr.rng_of("dirty_durations")
    B, L, T = 3, 9, 40
    lens = np.array([9, 5, 1], np.int32)
    nan, inf = np.float32("nan"), np.float32("inf")
    dirty = np.array([[3.0, nan, 2.75, -4.0, 0.0, 4.0, -inf, 1.999, 6.0],    # row sums of the clamped values stay <= T
                      [0.0, 0.0, 7.5, -0.0, 2.0, 5.0, nan, inf, 11.0],                 # zeros before a phoneme: the in-place path; junk past len 5
                      [0.5, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0]], np.float32)      # a fraction below 1 is 0: an empty utterance
    clean = np.array([[3, 0, 2, 0, 0, 4, 0, 1, 6], [0, 0, 7, 0, 2, 0, 0, 0, 0], [0] * 9], np.float32)
    frames = rng.standard_normal((B, T)).astype(np.float32)
    uvf = (rng.random((B, T)) > 0.5).astype(np.float32)
    uvf[0, :3] = 1.0   # phoneme 0 of row 0: mean exactly 1

    def scan(dur, mel_given=None, targets=True):
        d = torch.from_numpy(dur.copy()).cuda()
        tl = torch.from_numpy(lens).cuda()
        cum = torch.full((B, L), -7, dtype=torch.int32, device="cuda")
        m64 = torch.zeros(B, dtype=torch.int64, device="cuda")
        m32 = torch.zeros(B, dtype=torch.int32, device="cuda")
        src = [torch.from_numpy(frames).cuda(), torch.from_numpy(uvf).cuda()]
        dst = [torch.full((B, L), float("nan"), device="cuda") for _ in range(2)]
        srcs = (C.c_void_p * 2)(*[t.data_ptr() for t in src])
        dsts = (C.c_void_p * 2)(*[t.data_ptr() for t in dst])
        given = None if mel_given is None else torch.from_numpy(np.asarray(mel_given, np.int64)).cuda()
        msg = lib.e2ekt_teacher_scan(d.data_ptr(), tl.data_ptr(), cum.data_ptr(), m64.data_ptr(), m32.data_ptr(), None if given is None else given.data_ptr(),
                                     2 if targets else 0, srcs, dsts, (C.c_int * 2)(0, 1), B, L, T, None)
        assert msg is None, msg
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (d, cum, m64, m32, dst[0], dst[1])]

    d, cum, m64, m32, means, uv = scan(dirty)
    np.testing.assert_array_equal(d, clean)
    np.testing.assert_array_equal(cum, np.cumsum(clean.astype(np.int64), 1))
    np.testing.assert_array_equal(m64, clean.astype(np.int64).sum(1))
    np.testing.assert_array_equal(m32, m64)
    assert int(m64.max()) <= T
    np.testing.assert_array_equal(means.view(np.uint32), fr.get_phoneme_level(frames, lens, clean, L).view(np.uint32))
    uv_means = fr.get_phoneme_level(uvf, lens, clean, L)
    np.testing.assert_array_equal(uv, np.where(uv_means == 1.0, 1.0, 0.0).astype(np.float32))
    assert uv[0, 0] == 1.0
    for got, want in zip(scan(clean), (d, cum, m64, m32, means, uv)):   # the same bits as from durations that were clean to begin with
        np.testing.assert_array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want)
    # the cap, without targets (their frames end at T): inf and 3e6 count as 2^20; given mel lengths are clamped to [0, T]
    big = clean.copy()
    big[0, 8], big[1, 4] = inf, 3.0e6
    d, cum, m64, m32, _, _ = scan(big, mel_given=[T + 5, -3, 17], targets=False)
    want = clean.copy()
    want[0, 8] = want[1, 4] = 1048576.0
    np.testing.assert_array_equal(d, want)
    np.testing.assert_array_equal(cum, np.cumsum(want.astype(np.int64), 1))
    np.testing.assert_array_equal(m64, [T, 0, 17])
    np.testing.assert_array_equal(m32, [T, 0, 17])


def test_soft_mode_with_every_array_in_device_memory():
    """mel_lens, durations, map and targets in device memory: nothing is validated or known on the host, every utterance counts as T
    frames there (padded launch grids) and the kernels mask by the device copy of the lengths.  Valid rows, lengths and discrete
    outputs equal the host-memory call's bit for bit, and the fixture's bars hold."""
    import torch
    g = fc.load("forced_tiny_b3")
    cfg, eng = engine_of(g)
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    B = g["ids"].shape[0]
    r0, mel0, post0 = run_forced(eng, g, 0)
    din0 = eng.fetch_tap("dec_in", (B, r0["T"], H))
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("s0_dur", "attn_soft", "mel_lens", "f0", "uv", "energy")}
    eng.poison_workspace()
    r1, mel1, post1 = run_forced(eng, g, 0, durations=dev["s0_dur"], attn_soft=dev["attn_soft"], mel_lens=dev["mel_lens"], f0=dev["f0"],
                                 uv=dev["uv"], energy=dev["energy"])
    din1 = eng.fetch_tap("dec_in", (B, r1["T"], H))
    assert r1["T"] == r0["T"]
    for k in ("dur", "mel_lens", "pitch_idx", "energy_idx"):
        np.testing.assert_array_equal(r1[k], r0[k], err_msg=k)
    for b, n in enumerate(g["mel_lens"]):
        np.testing.assert_array_equal(din1[b, :n], din0[b, :n])
        np.testing.assert_array_equal(mel1[b, :n], mel0[b, :n])
        np.testing.assert_array_equal(post1[b, :n], post0[b, :n])
    check_fixture(eng, cfg, g, 0, r1, mel1, post1)


@pytest.mark.parametrize("name", ["tiny_pctl_b3", "tiny_frame_pctl_b3", "tiny_nouv_pctl_b3"])
def test_null_struct_is_the_ctl_path(name):
    """All-NULL struct: array_equal with e2etts_acoustic_ctl on the inputs of every tiny_*pctl_b3 fixture (per-phoneme controls): the
    phoneme-level use_uv model, the frame-level one (indices and predictions are [B, T] taps, the per-phoneme controls expanded along cum)
    and the pitch_no_uv one (pitch_pred [B, L])."""
    from test_gpu_controls import engine_controls
    from test_gpu_parity import engine_for
    g = load_golden(name)
    cfg, eng = engine_for(g, name)
    eng.set_precision("fp32", "fp32")
    spk = np.array([int(g["speaker"])], np.int64)
    d, p, e = engine_controls(g)
    a = eng.acoustic(g["ids"], g["lens"], spk, d, p, e, want=WANT)
    mel_a = eng.fetch_mel(a["B"], a["T"])
    b = eng.acoustic_forced(g["ids"], g["lens"], spk, d_control=d, p_control=p, e_control=e, want=WANT)
    mel_b = eng.fetch_mel(b["B"], b["T"])
    assert a["T"] == b["T"]
    for k in WANT:   # at the frame level pitch_idx / energy_idx / pitch_pred / energy_pred are the [B, T] taps the binding fetches after the call
        assert k in a and k in b and a[k].shape == b[k].shape == g[k].shape, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(mel_a[0], mel_b[0])
    np.testing.assert_array_equal(mel_a[1], mel_b[1])
    for k in ("dur", "mel_lens", "pitch_idx", "energy_idx"):
        np.testing.assert_array_equal(b[k], g[k], err_msg=k)
    with pytest.raises(RuntimeError):   # no forced pass, no forced taps
        eng.fetch_tap("dec_in", (a["B"], a["T"], cfg["models"]["fastspeech2"]["encoder_hidden"]))


def test_predicted_durations_fed_back_give_the_predicted_run():
    """Durations taken from a predicted run and given back as `durations`, no targets: every output equals that run bit for bit."""
    g = fc.load("forced_tiny_b3")
    cfg, eng = engine_of(g)
    eng.set_precision("fp32", "fp32")
    eng.set_ragged(False)   # e2etts_acoustic computes the padded rows: compare like with like
    try:
        a = eng.acoustic(g["ids"], g["txt_lens"], g["speakers"], 1.0, 1.0, 1.0, want=WANT)
        mel_a = eng.fetch_mel(a["B"], a["T"])
        b = eng.acoustic_forced(g["ids"], g["txt_lens"], g["speakers"], durations=a["dur"], want=WANT)
        mel_b = eng.fetch_mel(b["B"], b["T"])
    finally:
        eng.set_ragged(True)
    assert a["T"] == b["T"] and a["T"] > 0
    for k in WANT:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(mel_a[0], mel_b[0])
    np.testing.assert_array_equal(mel_a[1], mel_b[1])


@pytest.mark.parametrize("si", [0, 1], ids=["soft", "hard"])
def test_ragged_equals_padded_on_valid_rows(si):
    """Rows past an utterance's end are skipped in ragged mode: with the workspaces poisoned in between, valid rows are bit-identical."""
    g = fc.load("forced_tiny_b3")
    cfg, eng = engine_of(g)
    try:
        eng.set_ragged(False)
        r0, mel0, post0 = run_forced(eng, g, si)
        eng.set_ragged(True)
        eng.poison_workspace()
        r1, mel1, post1 = run_forced(eng, g, si)
    finally:
        eng.set_ragged(True)
    assert r0["T"] == r1["T"]
    np.testing.assert_array_equal(r0["mel_lens"], r1["mel_lens"])
    assert int(r0["mel_lens"].min()) < r0["T"]
    for b, n in enumerate(r0["mel_lens"]):
        np.testing.assert_array_equal(mel0[b, :n], mel1[b, :n])
        np.testing.assert_array_equal(post0[b, :n], post1[b, :n])
    check_fixture(eng, cfg, g, si, r1, mel1, post1)


def test_one_utterance_alone_equals_its_row_in_the_batch():
    """Soft mode: the second utterance (7 phonemes, 33 frames) alone -- B = 1, L = 7, its map cut to its own 7 columns; T stays 70 so that
    both runs read the same (regenerated) position table -- against its row of the batch of three."""
    g = fc.load("forced_tiny_b3")
    cfg, eng = engine_of(g)
    H = cfg["models"]["fastspeech2"]["encoder_hidden"]
    r, mel, post = run_forced(eng, g, 0)
    B, L = g["ids"].shape
    din = eng.fetch_tap("dec_in", (B, r["T"], H))
    b, n, m = 1, int(g["txt_lens"][1]), int(g["mel_lens"][1])
    sub = dict(ids=g["ids"][b:b + 1, :n].copy(), txt_lens=g["txt_lens"][b:b + 1], speakers=g["speakers"][b:b + 1], mel_lens=g["mel_lens"][b:b + 1],
               attn_soft=np.ascontiguousarray(g["attn_soft"][b:b + 1, :, :n]), s0_dur=np.ascontiguousarray(g["s0_dur"][b:b + 1, :n]),
               f0=np.ascontiguousarray(g["f0"][b:b + 1]), uv=np.ascontiguousarray(g["uv"][b:b + 1]),
               energy=np.ascontiguousarray(g["energy"][b:b + 1]), p_control=g["p_control"])
    r1, mel1, post1 = run_forced(eng, sub, 0)
    assert r1["T"] == r["T"] and int(r1["mel_lens"][0]) == m
    np.testing.assert_array_equal(eng.fetch_tap("dec_in", (1, r["T"], H))[0, :m], din[b, :m])
    np.testing.assert_array_equal(mel1[0, :m], mel[b, :m])
    np.testing.assert_array_equal(post1[0, :m], post[b, :m])


def test_forward_end_to_end_and_vocoder_on_the_resident_mel():
    """UnsupervisedFastSpeech2.forward on forced_tiny_b3's 10-tuple (aligner library -> engine, on the device), both steps, against the
    fixture; then e2etts_vocoder(NULL) on the resident mel equals vocoding the fetched mel_post."""
    from e2e_tts_amd import packer
    from e2e_tts_amd.models import UnsupervisedFastSpeech2
    g = fc.load("forced_tiny_b3")
    cfg, ac, voc = fc.states_of(g, vocoder=True)
    fs = cfg["models"]["fastspeech2"]
    class WithVocoder(UnsupervisedFastSpeech2):   # an engine that can vocode its resident mel (api.TTS shares one the same way)
        def _pack(self, state):
            return packer.pack(self._dims_cache, state, voc)

    m = WithVocoder(fc.cfgmod.N_SYMBOLS, 4, cfg["audio"]["mel"]["channels"], fs, fc.STATS, device=0,
                    hop_length=cfg["audio"]["stft"]["hop_length"], hifigan_config=cfg["models"]["hifigan"])
    m.load_state_dict(ac)
    m.eval()
    with pytest.raises(NotImplementedError):
        m.forward()
    B, L = g["ids"].shape
    T = g["mel"].shape[1]
    p_t, e_t = fc.targets_of(g)
    inputs = (g["speakers"], g["ids"], g["mel"], None, p_t, e_t, g["txt_lens"], L, g["mel_lens"], T)
    bad = list(inputs)
    bad[8] = np.array([70, 6, 5], np.int64)   # 6 frames for 7 phonemes
    with pytest.raises(ValueError, match="mel_len 6 < txt_len 7"):
        m.forward(tuple(bad))
    for si, step in enumerate((0, 10 ** 9)):
        (mel, post, log_d, p_pred, e_pred, tl, tmask, out_lens, mmask, attn_out), (p_ret, e_ret) = m(inputs, step=step)
        pre = f"s{si}_"
        np.testing.assert_array_equal(attn_out[2].cpu().numpy(), g[pre + "dur"])
        np.testing.assert_array_equal(out_lens.cpu().numpy(), g[pre + "mel_lens"])
        assert fc.valid_mean_l1(attn_out[0][:, 0].cpu().numpy(), g["attn_soft"], g["mel_lens"]) < 1e-5
        assert fc.valid_mean_l1(post.cpu().numpy(), g[pre + "mel_post"], g["mel_lens"]) < HIP_BAR
        assert fc.valid_mean_l1(mel.cpu().numpy(), g[pre + "mel"], g["mel_lens"]) < HIP_BAR
        for b, n in enumerate(g["txt_lens"]):
            np.testing.assert_array_equal(p_ret["uv"].cpu().numpy()[b, :n], g[pre + "p_uv"][b, :n])
        assert fc.valid_mean_l1(p_ret["f0"].cpu().numpy(), g[pre + "p_f0"], g["txt_lens"]) < 1e-5
        assert fc.valid_mean_l1(e_ret.cpu().numpy(), g[pre + "e_tgt"], g["txt_lens"]) < 1e-5
        assert bool(mmask[1, 33]) and not bool(mmask[1, 32]) and tuple(tmask.shape) == (B, L)
        eng = m.engine
        eng.set_precision("fp32", "fp32")
        wav_res, _ = eng.vocoder(None, B, T, wav=True, pcm=False)
        wav_fed, _ = eng.vocoder(post.transpose(1, 2).contiguous(), B, T, channels_first=True, wav=True, pcm=False)
        np.testing.assert_array_equal(wav_res, wav_fed)
        assert np.abs(wav_res).max() > 0


def test_forward_audio_is_align_audio_followed_by_the_forced_pass():
    """Recordings -> mel -> alignment -> teacher-forced mels without leaving the device: the result equals handing align_audio's outputs
    to the engine by way of the host, bit for bit, in both expansion modes; the mel lengths are the front-end's."""
    import test_gpu_mel as tgm
    from e2e_tts_amd import models
    g = load_golden(tgm.mr.ALIGN_FIXTURE)
    cfg = fc.cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    state = fc.sw.make_acoustic_state(cfg, fc.STATS, 4, seed=3, mode="varied")
    state.update(tgm.fixture_state(g))
    m = models.UnsupervisedFastSpeech2(fc.cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, fc.STATS, device=0)
    m.load_state_dict(fc.sw.to_torch(state))
    B, L = g["ids"].shape
    T = int(g["mel_lens"].max())
    assert (g["mel_lens"] >= g["txt_lens"]).all()
    rng = kr.rng_of("forward_audio")
    p_t = {"f0": rng.standard_normal((B, T)).astype(np.float32), "uv": (rng.random((B, T)) > 0.6).astype(np.float32)}
    soft, hard, dur, logprob, energy = m.align_audio(g["speakers"], g["ids"], g["txt_lens"], g["pcm"], g["n_valid"], return_energy=True)
    eng = m.engine
    eng.set_precision("fp32", "fp32")
    for step in (0, 10 ** 9):
        (mel, post, log_d, p_pred, e_pred, tl, tmask, out_lens, mmask, attn_out), (p_ret, e_ret) = m.forward_audio(
            g["speakers"], g["ids"], g["txt_lens"], g["pcm"], g["n_valid"], p_targets=p_t, e_targets=energy, step=step)   # the front-end's energies, a device tensor
        np.testing.assert_array_equal(out_lens.cpu().numpy(), g["mel_lens"])
        np.testing.assert_array_equal(attn_out[2].cpu().numpy(), dur.cpu().numpy())
        kw = dict(attn_soft=soft[:, 0].cpu().numpy(), mel_lens=g["mel_lens"]) if step == 0 else {}
        r = eng.acoustic_forced(g["ids"], g["txt_lens"], g["speakers"], durations=dur.cpu().numpy(), f0=p_t["f0"], uv=p_t["uv"],
                                energy=energy.cpu().numpy(), pitch_frames=True, energy_frames=True, T=T, want=("mel_lens",), **kw)
        assert r["T"] == T
        mel2, post2 = eng.fetch_mel(B, T)
        for b, n in enumerate(g["mel_lens"]):
            np.testing.assert_array_equal(mel.cpu().numpy()[b, :n], mel2[b, :n])
            np.testing.assert_array_equal(post.cpu().numpy()[b, :n], post2[b, :n])
        assert np.isfinite(post2[0, :int(g["mel_lens"][0])]).all() and e_ret.shape == (B, L) and p_ret["f0"].shape == (B, L)


def test_refusals_come_back_as_value_errors_and_leave_the_engine_usable():
    """The library's own checks (host_logic.h: forced_check, run before anything is enqueued) through the binding: E2ETTS_EINVAL with the
    offending value in the message; the next valid call gives the fixture's results."""
    g = fc.load("forced_tiny_b3")
    cfg, eng = engine_of(g)
    ids, lens, spk = g["ids"], g["txt_lens"], g["speakers"]
    T = g["attn_soft"].shape[1]
    dur = g["s0_dur"].copy()
    dur[0, 3] = -2.0
    with pytest.raises(ValueError, match=r"durations\[0, 3\] = -2 is negative"):
        eng.acoustic_forced(ids, lens, spk, durations=dur)
    dur[0, 3] = 1.5
    with pytest.raises(ValueError, match=r"durations\[0, 3\] = 1.5 is not an integer"):
        eng.acoustic_forced(ids, lens, spk, durations=dur)
    with pytest.raises(ValueError, match="uv is NULL"):
        eng.acoustic_forced(ids, lens, spk, durations=g["s0_dur"], f0=g["f0"], pitch_frames=True, T=T)
    with pytest.raises(ValueError, match="pitch_no_uv = 0"):
        eng.acoustic_forced(ids, lens, spk, durations=g["s0_dur"], pitch=g["f0"], pitch_frames=True, T=T)
    with pytest.raises(ValueError, match="`durations`, which is NULL"):
        eng.acoustic_forced(ids, lens, spk, energy=g["energy"], energy_frames=True, T=T)
    with pytest.raises(ValueError, match="needs mel_lens"):
        eng.acoustic_forced(ids, lens, spk, durations=g["s0_dur"], attn_soft=g["attn_soft"])
    with pytest.raises(ValueError, match=r"mel_lens\[2\]=71 outside \[1, 70\]"):
        eng.acoustic_forced(ids, lens, spk, durations=g["s0_dur"], attn_soft=g["attn_soft"], mel_lens=np.array([70, 33, 71], np.int64))
    with pytest.raises(ValueError, match="sum to 71 frames"):
        longer = g["s0_dur"].copy()
        longer[0, 0] += 1
        eng.acoustic_forced(ids, lens, spk, durations=longer, energy=g["energy"], energy_frames=True, T=T)
    r, mel, mel_post = run_forced(eng, g, 0)
    check_fixture(eng, cfg, g, 0, r, mel, mel_post)
