"""The vocoder critic on the GPU (libe2etts_critic.so, include/e2etts_critic.h): the grouped MFMA kernel alone, the dense layers through
the stride fold, the whole networks against the reference's fixtures (tools/make_critic_goldens.py), and the contract's bit-for-bit
statements (fused = materialised, a row = its B = 1 call, int16 = its float32 conversion).

Bars.  A single launch is held per element to gamma_n S and in aggregate to 4 x the float32-numpy yardstick (tests/kernel_ref.py).  End to
end the bars come from the REFERENCE'S OWN float32 error, element-wise: per map rms(got - ref64) / rms(ref64) over the sampled elements
<= 4 x the same statistic of the reference's float32 map; per figure |got - ref64| <= 4 x the triangle-inequality bound the fixture
records from the reference's float32 maps."""
import os

import numpy as np
import pytest

from conftest import ROOT
import critic_ref as cr
import kernel_cases as kc
import kernel_ref as kr
from e2e_tts_amd import critic as crit, packer, synth_weights as sw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 2024
LOSSES = ("feature_loss_mpd", "feature_loss_msd", "disc_loss_mpd", "disc_loss_msd", "gen_loss_mpd", "gen_loss_msd")
MSD_GROUPED = [(128, 128, 41, 2, 4, 20), (128, 256, 41, 2, 16, 20), (256, 512, 41, 4, 16, 20), (512, 1024, 41, 4, 16, 20), (1024, 1024, 41, 1, 16, 20)]


@pytest.fixture(scope="module")
def state():
    return sw.synth_critic_state(SEED, crit.default_config())


@pytest.fixture(scope="module")
def blob(state):
    return packer.pack_critic(*state, crit.default_config())


@pytest.fixture(scope="module")
def critic(blob):
    c = crit.Critic()
    c.load_blob(blob)
    yield c
    c.close()


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def check_launch(got, case, yard32, what):
    """Both bars of one launch on the rows that exist; rows past a sequence's length must be exactly 0."""
    ref, S, to = case["ref"], case["S"], case["to"]
    mask = np.arange(ref.shape[1])[None, :] < to[:, None]
    assert np.all(got[:, :ref.shape[1]][~mask] == 0) and np.all(got[:, ref.shape[1]:] == 0), f"{what}: rows past the length are not 0"
    err = np.abs(got[:, :ref.shape[1]].astype(np.float64) - ref)[mask]
    bar, Sm = (kr.gamma(case["n"]) * S)[mask], S[mask]
    worst = float(np.max(err / np.maximum(bar, 1e-300)))
    print(f"{what}: worst err / bar {worst:.3g}", end="")
    assert np.all(np.isfinite(got)) and worst <= 1.0, f"{what}: worst err / bar {worst}"
    if err.size >= kr.AGG_MIN_ELEMS:   # the yardstick's statistic is taken on the first sequence, as kernel_ref takes it on the first utterances
        ys = kr.rel_rms(np.abs(yard32.astype(np.float64) - ref[0, :to[0]]), S[0, :to[0]])
        gs = kr.rel_rms(err, Sm)
        print(f", aggregate {gs:.3g} against yardstick {ys:.3g}", end="")
        assert gs <= kr.AGG_FACTOR * ys, f"{what}: aggregate {gs} > 4 x {ys}"
    print()


def grouped_cases():
    """Every grouped MSD layer, and the same per-group shape with a quarter of the groups where that still is a grouped layer."""
    out = []
    for cin, cout, k, s, g, pad in MSD_GROUPED:
        out.append(pytest.param((cin, cout, k, s, g, pad), id=f"full-{cin}to{cout}s{s}g{g}"))
        if g // 4 > 1:
            out.append(pytest.param((cin // 4, cout // 4, k, s, g // 4, pad), id=f"quarter-{cin // 4}to{cout // 4}s{s}g{g // 4}"))
    return out


@pytest.mark.parametrize("shape", grouped_cases())
def test_grouped_kernel_alone(critic, shape):
    """One launch per MSD grouped shape at T_out 1, 33 and 257, three ragged sequences, on guarded buffers whose input rows past a
    sequence's length hold NaN; the quarter table keeps the per-group shapes with a quarter of the groups."""
    cin, cout, k, s, g, pad = shape
    rng = kr.rng_of(f"critic_grouped_{shape}")
    w = (rng.standard_normal((cout, cin // g, k)) * np.sqrt(2.0 / (cin // g * k))).astype(np.float32)
    b = (0.05 * rng.standard_normal(cout)).astype(np.float32)
    wf = torch.from_numpy(packer.group_fragments(w, g)).cuda()
    assert np.array_equal(packer.group_fragments(w, g), cr.group_fragments(w, g))
    bt = torch.from_numpy(b).cuda()
    for t_out in (1, 33, 257):
        n0 = max(1, (t_out - 1) * s + k - 2 * pad)
        lens = np.array([n0, n0 // 2 + 1, 1], np.int32)
        x = rng.standard_normal((3, n0, cin)).astype(np.float32)
        xg = x.copy()
        for i, n in enumerate(lens):
            xg[i, n:] = np.nan
        cap = t_out + 3
        guard = 4096
        raw = torch.full((2 * guard + 3 * cap * cout,), 777.0, device="cuda")
        out = raw[guard:guard + 3 * cap * cout].view(3, cap, cout)
        for tm in (0, 64):
            out.fill_(float("nan"))
            critic.debug_grouped_conv(torch.from_numpy(xg).cuda(), torch.from_numpy(lens).cuda(), wf, bt, out, cin, cout, k, s, g, pad, 0.1, tm)
            critic.sync()
            got = out.cpu().numpy()
            assert torch.all(raw[:guard] == 777.0) and torch.all(raw[guard + 3 * cap * cout:] == 777.0), "guard words were written"
            if tm == 0:
                case = cr.conv_case(x, lens, w, b, s, g, pad, 0.1)
                assert case["to"][0] == t_out
                check_launch(got, case, cr.conv_eval32(x, lens, w, b, s, g, pad, 0.1), f"grouped {shape} T_out {t_out}")
                first = got
            else:
                assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), "the result depends on the tile"


@pytest.mark.parametrize("disc", [0, 4], ids=["p2", "p11"])
def test_dense_layers_through_the_fold(critic, state, disc):
    """MPD layers 2 to 5 (three of them stride 3, run as folded stride-1 conv_gemm launches) at n = 3001: every map against the map before
    it, as the library handed it out, under both bars of tests/kernel_ref.py on the FOLDED problem (the launch conv_gemm really ran); and the
    folded float64 reference against the strided convolution of the restatement."""
    g = golden("critic_n3001")
    critic.forward(g["y"], g["lens"])
    layers = crit.default_config()["mpd"]
    prev, _ = critic.fmap(disc, 0)
    for l in range(1, 5):
        cout, k, s, grp, pad = layers[l]
        w = packer.critic_effective_weight(state[0], f"discriminators.{disc}.convs.{l}")
        b = state[0][f"discriminators.{disc}.convs.{l}.bias"]
        got, t = critic.fmap(disc, l)
        x = np.ascontiguousarray(prev[0].transpose(2, 1, 0))            # [p, T, Cin]
        P, T, Cin = x.shape
        wf, q = packer.stride_fold(w, s, pad)
        rows = max(-(-T // s), int(t[0]))
        xf = np.zeros((P, rows * s, Cin), np.float32)
        xf[:, :T] = x
        c = dict(name=f"critic_fold_{disc}_{l}", B=P, T=rows, Cin=s * Cin, Cout=cout, KW=wf.shape[1], dil=1, pad=q, in_slope=1.0, act=kc.ACT_LRELU, act_slope=0.1,
                 zts=0, bias=True, res=False, accumulate=False, lens=[int(t[0])] * P, act_rows=None, out_div=1.0)
        d = dict(x=xf.reshape(P, rows, s * Cin), w=wf, bias=b, res=None, old=None)
        ref = kr.conv_reference(c, d, 0)
        direct = cr.conv_case(x, np.full(P, T), w, b, s, 1, pad, 0.1)
        assert direct["to"][0] == t[0] and np.allclose(ref["ref"][:, :t[0]], direct["ref"], rtol=1e-12, atol=1e-14)
        mine = np.zeros((P, rows, cout), np.float32)
        mine[:, :t[0]] = got[0].transpose(2, 1, 0)
        r = kr.check_conv(c, d, 0, mine, ref=ref)
        print(f"disc {disc} layer {l}: worst err / bar {r['elem_ratio']:.3g}, aggregate ratio {r['agg_ratio']}")
        assert r["ok"], r["why"]
        prev = got


def rel_rms(a, ref):
    return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300))


@pytest.mark.parametrize("name", ["critic_n2049", "critic_n3001", "critic_b3_n1501", "critic_n29", "critic_n12"])
def test_end_to_end_against_the_reference(critic, name):
    """Every map and every figure of the default networks against the reference's float64 run, under bars made of the reference's own
    float32 error.

    Measured on one MI355X: the worst map of a fixture lies at 0.45 to 0.54 of its bar, the worst figure at 0.24 to 0.54
    (profiles/critic/README.md has the table)."""
    g = golden(name)
    B = g["y"].shape[0]
    res = critic.run(g["y"], g["lens"], g["g"], g["lens"])
    sides = {}
    for side in ("y", "g"):
        critic.forward(g[side], g["lens"])
        sides[side] = {(d, l): critic.fmap(d, l)[0] for d in range(critic.n_disc) for l in range(len(critic.tables[d][2]))}
    worst_map = worst_fig = 0.0
    fails, row_bounds = [], []
    for (d, l), _ in sides["y"].items():
        idx = g[f"idx_{d}_{l}"]
        for side, key in (("y", "r"), ("g", "g")):
            got = sides[side][(d, l)]
            ref64, ref32 = g[f"{key}64_{d}_{l}"], g[f"{key}32_{d}_{l}"]
            assert np.array_equal(idx, np.arange(0, got.size, max(1, min(997, got.size // 64)))), f"map d{d} l{l} has {got.size} elements"
            mine, theirs = rel_rms(got.reshape(-1)[idx], ref64), rel_rms(ref32, ref64)
            ratio = mine / (4 * theirs) if theirs > 0 else (0.0 if mine == 0 else np.inf)
            worst_map = max(worst_map, ratio)
            if ratio > 1:
                fails.append(f"map {key} d{d} l{l}: {mine:.3g} against 4 x {theirs:.3g}")
    for b in range(B):
        r = res[b]
        assert r["status"] == 0
        for d in range(critic.n_disc):
            for l in range(len(critic.tables[d][2])):
                e, bar = abs(r["fm"][d][l] - g["fig64_fm"][b, d, l]), 4 * g["bound_fm"][b, d, l]
                worst_fig = max(worst_fig, e / bar if bar > 0 else (0.0 if e == 0 else np.inf))
                if e > bar:
                    fails.append(f"fm row {b} d{d} l{l}: {e:.3g} against {bar:.3g}")
            for j, k in enumerate(("d_real", "d_fake", "g_fake")):
                e, bar = abs(r[k][d] - g[f"fig64_{k}"][b, d]), 4 * g["bound_mom"][b, d, j]
                worst_fig = max(worst_fig, e / bar if bar > 0 else (0.0 if e == 0 else np.inf))
                if e > bar:
                    fails.append(f"{k} row {b} d{d}: {e:.3g} against {bar:.3g}")
        P = len(critic.config["periods"])
        fam = [slice(0, P), slice(P, critic.n_disc)]
        bounds = [2 * np.nansum(g["bound_fm"][b, fam[0]]), 2 * np.nansum(g["bound_fm"][b, fam[1]]),
                  g["bound_mom"][b, fam[0], :2].sum(), g["bound_mom"][b, fam[1], :2].sum(), g["bound_mom"][b, fam[0], 2].sum(), g["bound_mom"][b, fam[1], 2].sum()]
        row_bounds.append(bounds)
        for j, k in enumerate(LOSSES):
            e = abs(r[k] - g["fig64_loss"][b, j])
            worst_fig = max(worst_fig, e / (4 * bounds[j]))
            if e > 4 * bounds[j]:
                fails.append(f"{k} row {b}: {e:.3g} against {4 * bounds[j]:.3g}")
    if B > 1:   # equal lengths: the mean of the per-row figures is the reference's batch figure up to rounding
        for j, k in enumerate(LOSSES):
            mean = np.mean([res[b][k] for b in range(B)])
            assert abs(mean - g["batch64"][j]) <= 4 * np.mean([rb[j] for rb in row_bounds]), (k, mean, g["batch64"][j])
    print(f"{name}: worst map ratio {worst_map:.3g}, worst figure ratio {worst_fig:.3g} (1 = the bar)")
    assert not fails, "\n".join(fails)


def test_fused_figures_equal_the_materialised_maps_bit_for_bit(critic):
    g = golden("critic_n3001")
    res = critic.run(g["y"], g["lens"], g["g"], g["lens"])[0]
    maps = {}
    for side in ("y", "g"):
        critic.forward(g[side], g["lens"])
        maps[side] = [[critic.fmap(d, l)[0][0] for l in range(len(critic.tables[d][2]))] for d in range(critic.n_disc)]
    want = cr.ordered_figures(maps["y"], maps["g"])
    for d in range(critic.n_disc):
        assert res["fm"][d] == want["fm"][d], (d, res["fm"][d], want["fm"][d])
        for k in ("d_real", "d_fake", "g_fake"):
            assert res[k][d] == want[k][d], (k, d)
    P = len(critic.config["periods"])
    assert res["feature_loss_mpd"] == 2.0 * sum(v for f in want["fm"][:P] for v in f)


RAGGED = (1500, 2049, 2050, 3001)


def ragged_batch():
    rng = kr.rng_of("critic_ragged")
    y = np.clip(0.3 * rng.standard_normal((4, 3001)), -1, 1).astype(np.float32)
    gg = np.clip(y + 0.05 * rng.standard_normal((4, 3001)), -1, 1).astype(np.float32)
    return y, gg, np.array(RAGGED, np.int64)


def test_every_row_of_a_ragged_batch_equals_its_own_call(critic, blob):
    """n = 1500, 2049, 2050, 3001 in one batch against four B = 1 calls, and against the batch run under a workspace cap that splits it
    into passes of one pair: figures and raw scores, bit for bit.  What lies past a row's length (NaN here) is never read."""
    y, gg, lens = ragged_batch()
    for b, n in enumerate(lens):
        y[b, n:] = np.nan
        gg[b, n:] = np.nan
    whole = critic.run(y, lens, gg, lens)
    scores = [critic.fetch_scores(d, side) for d in range(critic.n_disc) for side in (0, 1)]
    capped = crit.Critic(dict(crit.default_config(), workspace_cap_bytes=1 << 20))
    capped.load_blob(blob)
    try:
        assert capped.run(y, lens, gg, lens) == whole
    finally:
        capped.close()
    for b, n in enumerate(lens):
        critic.poison_workspace()   # NaN patterns in every buffer: nothing may rest on what an earlier call left (the fold reads zero rows)
        alone = critic.run(y[b:b + 1, :n], lens[b:b + 1], gg[b:b + 1, :n], lens[b:b + 1])[0]
        assert alone == whole[b], b
        i = 0
        for d in range(critic.n_disc):
            for side in (0, 1):
                assert np.array_equal(critic.fetch_scores(d, side)[0].view(np.uint32), scores[i][b].view(np.uint32))
                i += 1
        assert all(np.isfinite(v) for f in alone["fm"] for v in f)


def test_unequal_lengths_set_the_status_bit_and_leave_the_neighbours_alone(critic):
    y, gg, lens = ragged_batch()
    whole = critic.run(y, lens, gg, lens)
    glens = lens.copy()
    glens[1] = 2000
    mixed = critic.run(y, lens, gg, glens)
    assert mixed[0] == whole[0] and mixed[2] == whole[2] and mixed[3] == whole[3]
    r = mixed[1]
    assert r["status"] & crit.ST_LENGTHS_DIFFER and r["lengths_differ"] and np.isnan(r["feature_loss_mpd"]) and np.isnan(r["feature_loss_msd"])
    assert all(np.isnan(v) for f in r["fm"] for v in f)
    assert r["d_real"] == whole[1]["d_real"] and all(np.isfinite(v) for v in r["d_fake"] + r["g_fake"])
    one = critic.scores(gg[1:2, :2000], glens[1:2])[0]
    assert one["status"] == crit.ST_ONE_SIDED and one["d_fake"] == r["d_fake"] and one["d_real"] == r["g_fake"]


def test_int16_input_equals_its_float32_conversion(critic):
    y, gg, lens = ragged_batch()
    yi, gi = np.round(y * 20000).astype(np.int16), np.round(gg * 20000).astype(np.int16)
    a = critic.run(yi, lens, gi, lens)
    b = critic.run(yi.astype(np.float32) / np.float32(32768.0), lens, gi.astype(np.float32) / np.float32(32768.0), lens)
    assert a == b
    c = critic.run(torch.from_numpy(yi).cuda(), lens, torch.from_numpy(gi).cuda(), lens)   # resident input
    assert c == a


def test_mirrors_return_the_reference_lists(state):
    """models.MultiPeriodDiscriminator / MultiScaleDiscriminator on one shared Critic: forward(y, y_hat) gives the reference's four lists in
    its shapes, and the fixture's sampled elements lie inside the map bars."""
    from e2e_tts_amd import models
    g = golden("critic_b3_n1501")
    mpd = models.MultiPeriodDiscriminator()
    msd = models.MultiScaleDiscriminator(critic=mpd.critic)
    mpd.load_state_dict(state[0]).eval()
    msd.load_state_dict(state[1]).eval()
    try:
        y, gg = torch.from_numpy(g["y"])[:, None, :], torch.from_numpy(g["g"])[:, None, :]
        d0 = 0
        for net, n in ((mpd, 5), (msd, 3)):
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = net(y, gg)
            assert len(y_d_rs) == len(y_d_gs) == len(fmap_rs) == len(fmap_gs) == n
            for i in range(n):
                d = d0 + i
                assert tuple(y_d_rs[i].shape) == g[f"sr32_{d}"].shape and tuple(y_d_gs[i].shape) == g[f"sg32_{d}"].shape and y_d_rs[i].is_cuda
                assert torch.equal(y_d_rs[i], fmap_rs[i][-1].flatten(1, -1))
                assert fmap_rs[i][0].dim() == (4 if net is mpd else 3) and fmap_rs[i][0].shape[0] == 3
                for maps, key in ((fmap_rs, "r"), (fmap_gs, "g")):
                    for l, m in enumerate(maps[i]):
                        idx = g[f"idx_{d}_{l}"]
                        assert np.array_equal(idx, np.arange(0, m.numel(), max(1, min(997, m.numel() // 64))))
                        ref64, ref32 = g[f"{key}64_{d}_{l}"], g[f"{key}32_{d}_{l}"]
                        assert rel_rms(m.cpu().numpy().reshape(-1)[idx], ref64) <= 4 * rel_rms(ref32, ref64), (key, d, l)
            d0 += n
    finally:
        mpd.critic.close()


def test_evaluate_vocoder_equals_the_chain_made_by_hand(tmp_path_factory):
    """TTS.evaluate_vocoder on a tiny synthetic checkpoint and quarter-width discriminators: finite figures, equal to Critic.run called by
    hand on device buffers (the front-end's mel through the engine's vocoder into a GPU tensor, the recording as a GPU tensor), for float32
    and for int16 recordings."""
    from test_gpu_denoiser_api import write_checkpoints
    from e2e_tts_amd import config as cfgmod
    from e2e_tts_amd.api import TTS
    cfg = cfgmod.tiny_config()
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=7, mode="varied")
    voc = sw.make_vocoder_state(cfg, seed=8)
    apath, vpath = write_checkpoints(tmp_path_factory.mktemp("ckpt"), cfg, ac, voc)
    tts = TTS(apath, vpath, max_len=60)
    narrow = crit.quarter_config()
    c = crit.Critic(narrow)
    c.load(*sw.synth_critic_state(5, narrow))
    hop, sr = tts.hop_length, tts.sample_rate
    rec_lens = np.array([hop * 40 + 5, hop * 23, hop * 31 + hop // 2])
    t = np.arange(hop * 41) / sr
    rec = np.stack([0.4 * np.sin(2 * np.pi * f * t) + 0.02 * kr.rng_of(f"evoc{f}").standard_normal(t.size) for f in (130.0, 180.0, 240.0)]).astype(np.float32)
    try:
        for x in (rec, np.rint(rec * 20000).astype(np.int16)):
            got = tts.evaluate_vocoder(x, rec_lens, c)
            r = tts._recording_chain()._default_stft().frontend.forward(x, rec_lens, want=("mel",))
            mel, ml = torch.from_numpy(r["mel"]).cuda(), r["mel_lens"]
            B, T = mel.shape[0], mel.shape[1]
            pcm = x.dtype == np.int16
            out = torch.empty((B, T * hop), dtype=torch.int16 if pcm else torch.float32, device="cuda")
            tts.engine.vocoder(mel, B, T, channels_first=False, wav=not pcm, pcm=pcm, out_wav=None if pcm else out, out_pcm=out if pcm else None)
            n = np.minimum(ml * hop, rec_lens)
            want = c.run(torch.from_numpy(x).cuda(), n, out, n)
            assert got == want and len(got) == 3
            for r in got:
                assert r["status"] == 0 and all(np.isfinite(v) and v > 0 for f in r["fm"] for v in f)
                assert all(np.isfinite(r[k]) for k in LOSSES) and r["feature_loss_mpd"] > 0
    finally:
        c.close()
