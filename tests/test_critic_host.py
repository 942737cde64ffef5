"""The vocoder critic, the parts that need no GPU: the float64 restatement (tests/critic_ref.py) against the reference's float64 fixtures,
the stride fold against a strided convolution, the packer's folds against the weights the reference's modules computed, the length
formulas against the shapes torch produced, the bars of tests/test_gpu_critic.py on the reference's own float32 result and on mutations
of the restatement, and the companion library's C ABI -- its exports and the refusals that come before a device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import critic_ref as cr
from e2e_tts_amd import critic as crit, packer, synth_weights as sw

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 2024
CFG = crit.default_config()


@pytest.fixture(scope="module")
def state():
    return sw.synth_critic_state(SEED, CFG)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_critic_hash() != g.critic_hash() or g.built_critic_hash(g.CRITIC["test_lib"]) != g.critic_hash():
        g.build()
    return crit.load_library()


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def one_disc(x, state, d, mut=None):
    kind, idx, layers = crit.disc_tables(CFG)[d]
    w = cr.layer_weights(state[0] if kind == "mpd" else state[1], idx, layers, mut)
    x = np.asarray(x, np.float64)
    if kind == "mpd":
        return cr.forward_disc(x, w, layers, CFG["slope"], period=CFG["periods"][idx], mut=mut)
    return cr.forward_disc(x, w, layers, CFG["slope"], scale=idx, mut=mut)


def test_the_fixtures_belong_to_the_seeded_state(state):
    import hashlib
    h = hashlib.sha256()
    for sd in state:
        for k in sorted(sd):
            h.update(k.encode() + b"\0" + np.ascontiguousarray(sd[k]).tobytes())
    for name in ("critic_n2049", "critic_n3001", "critic_b3_n1501", "critic_n29", "critic_n12"):
        g = golden(name)
        assert bytes(g["state_hash"]).decode() == h.hexdigest()[:16] and int(g["seed"]) == SEED
        assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 1 << 20


def test_synth_state_is_seeded_and_bounded(state):
    again = sw.synth_critic_state(SEED, CFG)
    other = sw.synth_critic_state(SEED + 7, CFG)
    for a, b, c in zip(state, again, other):
        assert list(a) == sorted(a) == list(b)
        assert all(np.array_equal(a[k], b[k]) for k in a) and any(not np.array_equal(a[k], c[k]) for k in a)
    v = state[1]["discriminators.1.convs.3.weight_v"]
    assert v.shape == (512, 16, 41) and abs(float(v.std()) - np.sqrt(2.0 / (1.01 * 16 * 41))) < 0.01 * float(v.std())
    assert "discriminators.0.convs.0.weight_orig" in state[1] and "discriminators.0.convs.0.weight_g" not in state[1]
    assert state[0]["discriminators.4.conv_post.weight_v"].shape == (1, 1024, 3, 1)


@pytest.mark.parametrize("name", ["critic_n2049", "critic_n29", "critic_n12"])
def test_restatement_against_the_float64_fixtures(state, name):
    """Default widths, n = 2049 and the short n = 29 and 12: every sampled map ELEMENT within 1e-10 of itself and every figure within 1e-10 of
    itself.  One floor, from the number format and not from this code: a figure that is a difference of float64 numbers cannot be known
    better than their last places, so the bar of an fm entry is max(1e-10 x the figure, 4 ulp64 of the maps' mean magnitude).  The floor
    decides for one entry only, fm[5][7] at n = 12: both rows' single scores are 0.02 and differ by 1.06e-08, so 1e-10 of the figure
    (1e-18) lies below half a last place of either score (1.7e-18); the restatement sits 2.6e-09 of the figure (2.8e-17) from the
    reference there, and within 1e-10 everywhere else -- at n = 29 without the floor mattering at all."""
    g = golden(name)
    mr = cr.forward_all(g["y"][0], CFG, *state)
    mg = cr.forward_all(g["g"][0], CFG, *state)
    for d in range(8):
        for l in range(len(mr[d])):
            idx = g[f"idx_{d}_{l}"]
            for maps, key in ((mr, "r64"), (mg, "g64")):
                ref = g[f"{key}_{d}_{l}"]
                assert maps[d][l].size > idx[-1]
                assert np.all(np.abs(maps[d][l].reshape(-1)[idx] - ref) <= 1e-10 * np.abs(ref)), (d, l, key)
    f = cr.figures(mr, mg, 5)
    floored = []
    for d in range(8):
        for l in range(len(mr[d])):
            fig = g["fig64_fm"][0, d, l]
            floor = 4 * np.finfo(np.float64).eps * float(np.mean(np.abs(mr[d][l])) + np.mean(np.abs(mg[d][l])))
            assert abs(f["fm"][d][l] - fig) <= max(1e-10 * fig, floor), (d, l)
            if abs(f["fm"][d][l] - fig) > 1e-10 * fig:
                floored.append((d, l))
        for k in ("d_real", "d_fake", "g_fake"):
            assert abs(f[k][d] - g[f"fig64_{k}"][0, d]) <= 1e-10 * g[f"fig64_{k}"][0, d], (k, d)
    assert floored == ([(5, 7)] if name == "critic_n12" else []), floored
    for j, k in enumerate(("feature_loss_mpd", "feature_loss_msd", "disc_loss_mpd", "disc_loss_msd", "gen_loss_mpd", "gen_loss_msd")):
        assert abs(f[k] - g["fig64_loss"][0, j]) <= 1e-10 * g["fig64_loss"][0, j], k


def test_length_formulas_against_the_shapes_torch_produced():
    g = golden("critic_n2049")
    want = [26, 27, 30, 28, 33, 33, 17, 9]
    for d, (kind, idx, layers) in enumerate(crit.disc_tables(CFG)):
        lens = cr.disc_lens(2049, layers, period=CFG["periods"][idx] if kind == "mpd" else 0, scale=idx if kind == "msd" else 0)
        cols = CFG["periods"][idx] if kind == "mpd" else 1
        assert lens[-1] * cols == want[d] == g[f"sr32_{d}"].size
    g = golden("critic_n12")
    for d, (kind, idx, layers) in enumerate(crit.disc_tables(CFG)):
        lens = cr.disc_lens(12, layers, period=CFG["periods"][idx] if kind == "mpd" else 0, scale=idx if kind == "msd" else 0)
        assert lens[-1] * (CFG["periods"][idx] if kind == "mpd" else 1) == g[f"sr32_{d}"].size


FOLDS = sorted({(k, s, p) for _, k, s, grp, p in CFG["mpd"] + CFG["msd"] if grp == 1} | {(7, 4, 1), (3, 5, 0)})


@pytest.mark.parametrize("k,s,pad", FOLDS)
def test_stride_fold_against_a_strided_convolution(k, s, pad):
    rng = np.random.default_rng(k * 100 + s * 10 + pad)
    Cin, Cout = 3, 5
    w = rng.standard_normal((Cout, Cin, k))
    b = rng.standard_normal(Cout)
    wf, q = packer.stride_fold(w.astype(np.float32), s, pad)
    wf64, q64 = cr.stride_fold(w, s, pad)
    assert q == q64 and np.array_equal(wf, wf64.astype(np.float32))
    assert np.count_nonzero(wf64) == w.size                      # every tap lands exactly once
    assert abs(cr.fold_waste(k, s, pad) - (1 - w.size / wf64.size)) < 1e-15
    for T in list(range(max(1, k - 2 * pad), 40)) + [97]:
        x = rng.standard_normal((T, Cin))
        direct = cr.conv1d(x, w, b, s, 1, pad)
        folded = cr.folded_conv(x, wf64, q, s)[:direct.shape[0]] + b
        assert direct.shape[0] == cr.out_len(T, k, s, pad) and np.allclose(direct, folded, rtol=1e-13, atol=1e-13), T
    if (k, s, pad) == (5, 3, 2):
        assert wf64.shape[1] == 2 and abs(cr.fold_waste(k, s, pad) - 1 / 6) < 1e-15


def test_pack_critic_folds_against_the_reference_modules(state):
    """weight_norm and the spectral-norm sigma (no power iteration) exactly as the reference's eval() forward computed them; the float64
    restatement agrees to float32 rounding; one more power iteration does not."""
    g = golden("critic_n2049")
    for d, (kind, idx, layers) in enumerate(crit.disc_tables(CFG)):
        sd = state[0] if kind == "mpd" else state[1]
        for l in range(len(layers)):
            prefix = f"discriminators.{idx}." + ("conv_post" if l == len(layers) - 1 else f"convs.{l}")
            widx, want = g[f"widx_{d}_{l}"], g[f"w_{d}_{l}"]
            got = packer.critic_effective_weight(sd, prefix)
            assert got.shape == (layers[l][0], (1 if l == 0 else layers[l - 1][0]) // layers[l][3], layers[l][1])
            assert np.array_equal(got.reshape(-1)[widx], want), (d, l)
            mine = cr.effective_weight(sd, prefix).reshape(-1)[widx]
            # (torch folds in float32: a norm over up to 5120 squares, a division and a product -- a few units in the last place of the largest weight)
            assert np.max(np.abs(mine - want)) <= 32 * 2.0 ** -24 * np.max(np.abs(want)), (d, l)
            if kind == "msd" and idx == 0 and l == 3:
                other = cr.effective_weight(sd, prefix, mut="sigma_iter").reshape(-1)[widx]
                assert np.max(np.abs(other - want)) > 1000 * 2.0 ** -24 * np.max(np.abs(want))
    bad = dict(state[1])
    bad["discriminators.0.convs.2.weight_u"] = np.zeros_like(bad["discriminators.0.convs.2.weight_u"])
    with pytest.raises(ValueError, match="sigma is 0"):
        packer.pack_critic_tensors(state[0], bad, CFG)
    bad["discriminators.0.convs.2.weight_u"] = np.full_like(bad["discriminators.0.convs.2.weight_u"], np.inf)
    with pytest.raises(ValueError, match="sigma is"):
        packer.pack_critic_tensors(state[0], bad, CFG)


def test_pack_critic_layouts(state):
    t = packer.pack_critic_tensors(*state, CFG)
    assert list(t)[:2] == ["d0.l0.w", "d0.l0.b"] and len(t) == 2 * (5 * 6 + 3 * 8)
    assert t["d0.l0.w"].size == 32 * 5 and t["d0.l1.w"].size == 128 * 2 * 96 and t["d0.l4.w"].size == 1024 * 5 * 1024 and t["d0.l5.w"].size == 3 * 1024
    assert t["d5.l1.w"].size == 128 * 32 * 41 and t["d5.l2.w"].size == 2 * 256 * 8 * 41 and t["d5.l6.w"].size == 1024 * 5 * 1024
    w = packer.critic_effective_weight(state[1], "discriminators.1.convs.2")
    assert np.array_equal(t["d6.l2.w"], cr.group_fragments(w, 16))
    w = packer.critic_effective_weight(state[0], "discriminators.2.convs.1")
    assert np.array_equal(t["d2.l1.w"].reshape(128, 2, 96), cr.stride_fold(w, 3, 2)[0])
    w = packer.critic_effective_weight(state[0], "discriminators.2.convs.3")     # Cin' = 1536, K' = 2: eight ranges of 192 channels
    wf = cr.stride_fold(w, 3, 2)[0]
    assert packer.dense_splits(1536, 2) == 8 and packer.dense_splits(384, 2) == 4 and packer.dense_splits(96, 2) == 1 and packer.dense_splits(1024, 5) == 8
    got = t["d2.l3.w"].reshape(8, 1024, 2, 192)
    assert all(np.array_equal(got[i], wf[:, :, 192 * i:192 * (i + 1)]) for i in range(8))
    assert np.array_equal(t["d2.l5.w"].reshape(3, 1024), packer.critic_effective_weight(state[0], "discriminators.2.conv_post")[0].T)
    narrow = crit.quarter_config()
    tq = packer.pack_critic_tensors(*sw.synth_critic_state(SEED, narrow), narrow)
    assert tq["d5.l1.w"].size == 32 * 21 * 2 * 32 and tq["d5.l2.w"].size == 4 * 1 * 41 * 4 * 64   # a dense k 41 stride 2 fold; 16-column groups in 32-column tiles


def test_ordered_sum_is_the_header_order_word_for_word():
    """Against a scalar loop written from the header's sentence, bit for bit; and against the plain sum up to rounding."""
    def tree(v):
        v = list(v)
        s = 128
        while s >= 1:
            for i in range(s):
                v[i] = v[i] + v[i + s]
            s //= 2
        return v[0]

    def slow(vals):
        nch = -(-len(vals) // 4096)
        lanes = [0.0] * 256
        for c in range(nch):
            lane = [0.0] * 256
            for e in range(c * 4096, min(len(vals), (c + 1) * 4096)):
                lane[e % 256] = lane[e % 256] + float(vals[e])
            lanes[c % 256] = lanes[c % 256] + tree(lane)
        return tree(lanes)
    rng = np.random.default_rng(5)
    for n in (1, 255, 257, 4096, 4097, 9001):
        v = rng.standard_normal(n) ** 2
        assert cr.ordered_sum(v) == slow(v), n
    for n in (70000, 4096 * 257 + 3):
        v = rng.standard_normal(n) ** 2
        assert abs(cr.ordered_sum(v) - v.sum()) <= 1e-12 * v.sum()


def judge(g, d, maps_r, maps_g):
    """The bars of tests/test_gpu_critic.py on one discriminator's maps (float64 or float32, the reference's layout): what fails."""
    fails = []
    for l in range(len(maps_r)):
        idx = g[f"idx_{d}_{l}"]
        for maps, key in ((maps_r, "r"), (maps_g, "g")):
            ref64, ref32 = g[f"{key}64_{d}_{l}"], g[f"{key}32_{d}_{l}"]
            rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref64) ** 2)))  # noqa: E731
            if rms(maps[l].reshape(-1)[idx]) > 4 * rms(ref32):
                fails.append(f"map {key} l{l}")
        if abs(np.mean(np.abs(maps_r[l].astype(np.float64) - maps_g[l])) - g["fig64_fm"][0, d, l]) > 4 * g["bound_fm"][0, d, l]:
            fails.append(f"fm l{l}")
    sr, sg = maps_r[-1].astype(np.float64), maps_g[-1].astype(np.float64)
    for j, (k, v) in enumerate((("d_real", np.mean((1 - sr) ** 2)), ("d_fake", np.mean(sg ** 2)), ("g_fake", np.mean((1 - sg) ** 2)))):
        if abs(v - g[f"fig64_{k}"][0, d]) > 4 * g["bound_mom"][0, d, j]:
            fails.append(k)
    return fails


def test_bars_pass_the_reference_float32_result():
    """The reference's own float32 run lies inside every bar: its maps by construction (a quarter of the map bar), its means -- evaluated
    in float64 from its float32 maps, as the library evaluates them -- because the bars are bounds of exactly that difference; the second
    order term of a squared score is what the factor 4 leaves room for."""
    for name in ("critic_n2049", "critic_n3001", "critic_b3_n1501", "critic_n29", "critic_n12"):
        g = golden(name)
        for b in range(g["y"].shape[0]):
            for d in range(8):
                for l in range(8):
                    if not np.isnan(g["fig64_fm"][b, d, l]):
                        assert abs(g["fig32d_fm"][b, d, l] - g["fig64_fm"][b, d, l]) <= g["bound_fm"][b, d, l] * (1 + 1e-9), (name, b, d, l)
                for j, k in enumerate(("d_real", "d_fake", "g_fake")):
                    assert abs(g["fig32d_mom"][b, d, j] - g[f"fig64_{k}"][b, d]) <= 4 * g["bound_mom"][b, d, j], (name, k, b, d)


@pytest.mark.parametrize("mut,d", [(None, 6), ("drop_tap", 6), ("pre_activation", 0), ("reflect_repeat", 0), ("pool_divisor", 6), ("sigma_iter", 5)])
def test_bars_fail_the_listed_mutations(state, mut, d):
    """The restatement of one discriminator at n = 2049, unmutated (inside every bar) and with one thing wrong (outside at least one)."""
    g = golden("critic_n2049")
    fails = judge(g, d, one_disc(g["y"][0], state, d, mut), one_disc(g["g"][0], state, d, mut))
    if mut is None:
        assert not fails, fails
    else:
        assert fails, f"the bars do not see {mut}"


def test_header_bindings_and_exports_agree(lib):
    import __graft_entry__ as g
    hdr = open(g.CRITIC["hdr"]).read()
    product, hooks = hdr.split("#ifdef E2ECR_TEST_HOOKS")
    decl = lambda text: re.findall(r"E2ECR_API\s+[\w\s\*]+?\b(e2ecr_\w+)\s*\(", text)  # noqa: E731
    assert decl(product) == crit.EXPORTED_SYMBOLS and len(crit.EXPORTED_SYMBOLS) == 17
    assert decl(hooks) == crit.TEST_HOOK_SYMBOLS and len(crit.TEST_HOOK_SYMBOLS) == 2
    for path, want in ((g.CRITIC["lib"], set(crit.EXPORTED_SYMBOLS)), (g.CRITIC["test_lib"], set(crit.EXPORTED_SYMBOLS + crit.TEST_HOOK_SYMBOLS))):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if " T " in ln} == want, path
    assert g.critic_hash() in lib.e2ecr_version().decode() and lib.e2ecr_abi_version() == crit.ABI_VERSION
    assert any(os.path.basename(f) == "plan.h" for f in g.CRITIC["extra"]) and g.CRITIC in g.COMPANIONS
    import ctypes as C
    c = crit.CConfig()
    lib.e2ecr_default_config(C.byref(c))
    mine = crit._c_config(CFG)
    assert bytes(c) == bytes(mine) and C.sizeof(crit.CConfig) == 424 and crit.RESULT_DTYPE.itemsize == 16 + 8 * (12 * 9 + 36 + 6)


def test_bad_tables_are_refused_by_name(lib):
    def refuse(match, **kw):
        with pytest.raises(ValueError, match=match):
            crit.Critic(dict(CFG, **kw))
    refuse("Cin / groups must be a multiple of 8", msd=[(128, 15, 1, 1, 7), (128, 41, 2, 32, 20)])
    refuse("Cout / groups must be a multiple of 16", msd=[(128, 15, 1, 1, 7), (160, 41, 2, 4, 20)])
    refuse("groups must divide", msd=[(128, 15, 1, 1, 7), (128, 41, 2, 3, 20)])
    refuse("scale discriminator layer 1: .*64 KiB", msd=[(1024, 15, 1, 1, 7), (1024, 41, 8, 2, 20)])
    refuse("period discriminator layer 1: dense layer", mpd=[(32, 5, 3, 1, 2), (30, 5, 3, 1, 2)])
    refuse("post layer", mpd_post=(2, 3, 1, 1, 1))
    refuse("periods must lie", periods=[2, 0])
    refuse("slope", slope=1.5)
    refuse("at least one discriminator", periods=[], n_scales=0)


def test_wrappers_refuse_bad_arguments_before_launching(lib):
    """Nothing here opens a device: every refusal comes from validation."""
    c = crit.Critic()
    y = np.zeros((2, 64), np.float32)
    lens = np.array([64, 64])
    with pytest.raises(ValueError, match="lens: 1 elements"):
        c.run(y, lens[:1], y, lens)
    with pytest.raises(ValueError, match="y and g differ"):
        c.run(y, lens, y[:1], lens[:1])
    with pytest.raises(ValueError, match="longer than ld .*g_lens\\[0\\] = 64.*ld 32"):
        c.run(y, lens, y[:, :32], lens)          # each side has its own row stride
    with pytest.raises(ValueError, match="y and g differ"):
        c.run(y, lens, y.astype(np.int16), lens)
    with pytest.raises(ValueError, match="expected samples of shape"):
        c.run(y[0], lens, y, lens)
    with pytest.raises(ValueError, match="shorter than the smallest accepted length .*g_lens\\[1\\] = 11"):
        c.run(y, lens, y, np.array([64, 11]))
    with pytest.raises(ValueError, match="longer than ld"):
        c.scores(y, np.array([64, 65]))
    with pytest.raises(RuntimeError, match="before e2ecr_load_weights"):
        c.run(y, lens, y, lens)
    with pytest.raises(RuntimeError, match="before e2ecr_load_weights"):
        c.forward(y, lens)
    import torch
    with pytest.raises(TypeError, match="expected float32 or int16"):
        c.scores(torch.zeros(2, 64, dtype=torch.float64), lens)
    with pytest.raises(ValueError, match="weight blob too small"):
        c.load_blob(np.zeros(8, np.uint8))
    rc = lib.e2ecr_run(c._h, None, lens.ctypes.data, 64, None, None, 0, 2, 0, None)
    assert rc == crit.E_INVAL and b"must not be NULL" in lib.e2ecr_last_error(c._h)
    rc = lib.e2ecr_run(c._h, y.ctypes.data, lens.ctypes.data, 64, y.ctypes.data, None, 64, 2, 0, None)
    assert rc == crit.E_INVAL and b"both be given" in lib.e2ecr_last_error(c._h)
    for B, ld, dt in ((0, 64, 0), (4097, 64, 0), (2, 0, 0), (2, 64, 7)):
        assert lib.e2ecr_run(c._h, y.ctypes.data, lens.ctypes.data, ld, None, None, 0, B, dt, None) == crit.E_INVAL
    assert lib.e2ecr_fetch_fmap(c._h, 0, 0, None, None, None) == crit.E_STATE
    assert lib.e2ecr_fetch_scores(c._h, 0, 0, None, None, None) == crit.E_STATE
    assert lib.e2ecr_run(None, None, None, 1, None, None, 1, 1, 0, None) == crit.E_INVAL and c.device_bytes() == 0
    narrow = sw.synth_critic_state(SEED, crit.quarter_config())
    with pytest.raises(ValueError, match="weight of shape"):
        packer.pack_critic(*narrow, CFG)
    c.close()
