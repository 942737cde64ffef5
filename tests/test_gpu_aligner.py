"""GPU tests (-m gpu) of forced alignment on the HIP path (include/e2etts_align.h, e2e_tts_amd/aligner.py, models.AlignmentEncoder / b_mas /
UnsupervisedFastSpeech2.align) against the reference's fixtures (tools/make_aligner_goldens.py) and, where no fixture exists, against the
numpy restatement (tests/aligner_ref.py).

Bars.  The search is additions and comparisons of fp32 in a fixed order: given the same log map it must give the reference's path bit for
bit -- no tolerance.  The forward differs from torch's CPU kernels in summation order only: mean / max |HIP - reference float64| over the valid
region stay within 4 x / 8 x the reference's own |fp32 - float64| on the same fixture (the denoiser tests' margin).  Durations end to end are
compared exactly on fixtures whose path survived the tool's robustness screen (noise of 16 x the fp32 error on the log map, 32 times).

Measured on an MI355X (HIP vs reference float64; the reference's own fp32 in brackets) -- see profiles/aligner/README.md."""
import numpy as np
import pytest

from conftest import load_golden
import aligner_ref as ar
from aligner_cases import FORWARD_FIXTURES, MAX_BAR, MEAN_BAR, fixture_inputs, fixture_state
from e2e_tts_amd import aligner as al, config as cfgmod, packer, synth_weights as sw

pytestmark = pytest.mark.gpu

_HANDLES, _RUNS = {}, {}


def handle_for(g, state):
    key = (int(g["hidden"]), int(g["n_mel"]), float(g["temperature"]), int(g["weight_seed"]), float(g["weight_scale"]))
    if key not in _HANDLES:
        h = al.Aligner(key[1], key[1], key[0], key[2], device=0)
        h.load_weights(packer.pack_aligner(state))
        _HANDLES[key] = h
    return _HANDLES[key]


def run_fixture(name):
    """One e2ealign_align call per fixture (host arrays in, every output out), shared by the tests below and left unchanged."""
    if name not in _RUNS:
        g = load_golden(name)
        state, keys, spk, prior = fixture_inputs(g)
        h = handle_for(g, state)
        r = h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], prior, want=("dur", "attn_hard", "attn", "attn_logprob"))
        _RUNS[name] = (g, h, keys, spk, prior, r)
    return _RUNS[name]


def check_bars(tag, attn, logprob, attn64, logprob64, ref_a, ref_l, cols, mel_lens):
    ea = ar.valid_stats(attn, attn64, cols, mel_lens)
    el = ar.valid_stats(logprob, logprob64, cols, mel_lens, full_columns=True)
    print(f"{tag}: attn mean {ea[0]:.3e} max {ea[1]:.3e} [reference fp32 {ref_a[0]:.3e} / {ref_a[1]:.3e}]; attn_logprob mean {el[0]:.3e} max {el[1]:.3e} "
          f"[reference fp32 {ref_l[0]:.3e} / {ref_l[1]:.3e}]")
    assert ea[0] <= MEAN_BAR * ref_a[0] and ea[1] <= MAX_BAR * ref_a[1], (ea, tuple(ref_a))
    assert el[0] <= MEAN_BAR * ref_l[0] and el[1] <= MAX_BAR * ref_l[1], (el, tuple(ref_l))


def mas_handle():
    if "mas" not in _HANDLES:
        _HANDLES["mas"] = al.Aligner(4, 1, 4, 1.0, device=0)
    return _HANDLES["mas"]


@pytest.mark.parametrize("name", FORWARD_FIXTURES + ["mas:eq", "mas:short", "mas:plain"])
def test_mas_is_the_references_path_bit_for_bit(name):
    if name.startswith("mas:"):
        g, tag = load_golden("aligner_mas_only"), name[4:]
        attn, il, ol, hard, dur = (g[f"{tag}_{k}"] for k in ("attn", "in_lens", "out_lens", "attn_hard", "dur"))
    else:
        g = load_golden(name)
        attn, il, ol, hard, dur = g["attn"], g["txt_lens"], g["mel_lens"], g["attn_hard"], g["dur"]
    with np.errstate(divide="ignore"):
        loga = np.log(attn)            # fp32 on the host: the map the reference's search works on
    r = mas_handle().mas(loga, il, ol, log_map=True)
    assert np.array_equal(r["attn_hard"], hard.astype(np.float32))      # every row, padding included
    assert np.array_equal(r["dur"], dur)
    ok = ol >= il
    assert np.array_equal(r["dur"].sum(1)[ok], ol[ok].astype(np.float32))
    only_dur = mas_handle().mas(loga, il, ol, log_map=True, want=("dur",))   # attn_hard NULL
    assert np.array_equal(only_dur["dur"], dur)


@pytest.mark.parametrize("B,T,L,il,ol", [(2, 2100, 160, (160, 97), (2100, 1500)),     # one wavefront per row (L <= 256), back-pointer bits in the workspace
                                         (2, 320, 300, (300, 257), (320, 300)),       # rows wider than 256: the workgroup form and its column loop, bits in LDS
                                         (2, 1100, 300, (300, 64), (1100, 900)),      # the workgroup form with the bits in the workspace
                                         (1, 760, 700, (700,), (760,))])              # three columns per thread in the workgroup form (L > 512)
def test_mas_paths_no_fixture_reaches(B, T, L, il, ol):
    rng = np.random.Generator(np.random.PCG64(T + L))
    loga = np.log(rng.random((B, T, L)).astype(np.float32) ** 6 + np.float32(1e-30))
    il, ol = np.asarray(il, np.int64), np.asarray(ol, np.int64)
    want = ar.b_mas(loga, il, ol, log_map=True, search=ar.mas_rows)
    r = mas_handle().mas(loga, il, ol, log_map=True)
    assert np.array_equal(r["attn_hard"], want) and np.array_equal(r["dur"], want.sum(1))


@pytest.mark.parametrize("name", FORWARD_FIXTURES)
def test_forward_within_the_references_own_error(name):
    g, h, keys, spk, prior, r = run_fixture(name)
    check_bars(name, r["attn"], r["attn_logprob"], g["attn64"], g["attn_logprob64"], g["ref_err_attn"], g["ref_err_logprob"], g["txt_lens"], g["mel_lens"])
    for b, n in enumerate(g["txt_lens"]):
        assert not r["attn"][b, :, n:].any()                 # masked keys: exactly 0
        assert np.isfinite(r["attn_logprob"][b]).all()       # before the mask: finite everywhere (held to the bar above, all columns)
    assert np.allclose(r["attn"].sum(-1), 1.0, atol=1e-5)
    # e2ealign_forward gives the same bits as e2ealign_align, and leaves attn resident for a search with a NULL map
    f = h.forward(g["mel"], keys, spk, g["txt_lens"], prior)
    assert np.array_equal(f["attn"], r["attn"]) and np.array_equal(f["attn_logprob"], r["attn_logprob"])
    m = h.mas(None, g["txt_lens"], g["mel_lens"], B=r["attn"].shape[0], T=r["attn"].shape[1], L=r["attn"].shape[2])
    assert np.array_equal(m["attn_hard"], r["attn_hard"]) and np.array_equal(m["dur"], r["dur"])
    if "nomask_attn" in g:   # mask=None: nothing filled, the softmax over every column
        f = h.forward(g["mel"], keys, spk, None, prior)
        full = np.full(len(g["txt_lens"]), keys.shape[1])
        check_bars(name + " mask=None", f["attn"], f["attn_logprob"], g["nomask_attn64"], g["nomask_attn_logprob64"], g["nomask_ref_err_attn"],
                   g["nomask_ref_err_logprob"], full, g["mel_lens"])
    with pytest.raises(ValueError):
        h.mas(None, g["txt_lens"], g["mel_lens"], B=1, T=3, L=2)   # not the resident geometry


@pytest.mark.parametrize("name", FORWARD_FIXTURES)
def test_durations_end_to_end_equal_the_references(name):
    g, h, keys, spk, prior, r = run_fixture(name)
    assert np.array_equal(r["dur"], g["dur"])                                  # every row
    assert np.array_equal(r["attn_hard"], g["attn_hard"].astype(np.float32))
    ok = g["mel_lens"] >= g["txt_lens"]
    assert np.array_equal(r["dur"].sum(1)[ok], g["mel_lens"][ok].astype(np.float32))


@pytest.mark.parametrize("name", [n for n in FORWARD_FIXTURES if "noprior" not in n])
def test_model_align_gives_the_references_attn_out(name):
    """UnsupervisedFastSpeech2.align on a whole checkpoint: the aligner built from variance_adaptor.aligner.*, the embedding rows gathered
    with torch, the prior built per row (the reference has no attn_out without a prior, so the no-prior fixture has no counterpart here)."""
    import torch
    from e2e_tts_amd.models import UnsupervisedFastSpeech2
    g = load_golden(name)
    cfg = cfgmod.tiny_config()
    fs = cfg["models"]["fastspeech2"]
    fs["encoder_hidden"] = fs["decoder_hidden"] = int(g["hidden"])
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=3, mode="varied")
    state.update(fixture_state(g))                # the fixture's aligner, phoneme and speaker tables
    m = UnsupervisedFastSpeech2(cfgmod.N_SYMBOLS, 4, int(g["n_mel"]), fs, cfgmod.DEFAULT_STATS, device=0)
    m.load_state_dict(sw.to_torch(state))
    with pytest.raises(NotImplementedError, match="align"):
        m.forward()
    soft, hard, dur, logprob = m.align(torch.from_numpy(g["speakers"]), torch.from_numpy(g["ids"]), torch.from_numpy(g["txt_lens"]),
                                       torch.from_numpy(g["mel"]), torch.from_numpy(g["mel_lens"]))
    B, T, L = g["attn"].shape
    assert soft.shape == hard.shape == logprob.shape == (B, 1, T, L) and dur.shape == (B, L) and soft.is_cuda and dur.is_cuda
    assert np.array_equal(dur.cpu().numpy(), g["dur"])
    assert np.array_equal(hard[:, 0].cpu().numpy(), g["attn_hard"].astype(np.float32))
    r = run_fixture(name)[5]       # the same bits as the C entry point on host arrays
    assert np.array_equal(soft[:, 0].cpu().numpy(), r["attn"]) and np.array_equal(logprob[:, 0].cpu().numpy(), r["attn_logprob"])


def test_alignment_encoder_and_b_mas_mirrors():
    import torch
    from e2e_tts_amd.models import AlignmentEncoder, b_mas
    g, h, keys, spk, prior, r = run_fixture("aligner_tiny_b3")
    enc = AlignmentEncoder(int(g["n_mel"]), int(g["n_mel"]), int(g["hidden"]), float(g["temperature"]), device=0)
    enc.load_state_dict(sw.to_torch(ar.submodule_state(fixture_state(g))))
    L = keys.shape[1]
    mask = (torch.arange(L)[None, :] >= torch.from_numpy(g["txt_lens"])[:, None]).unsqueeze(-1)
    attn, logprob = enc(torch.from_numpy(g["mel"]).transpose(1, 2).cuda(), torch.from_numpy(keys).transpose(1, 2).cuda(), mask.cuda(),
                        torch.from_numpy(prior).cuda(), torch.from_numpy(spk).cuda())
    assert attn.is_cuda and attn.shape == (3, 1, 70, 12)
    assert np.array_equal(attn[:, 0].cpu().numpy(), r["attn"]) and np.array_equal(logprob[:, 0].cpu().numpy(), r["attn_logprob"])
    hard = b_mas(attn, g["txt_lens"], g["mel_lens"], width=1)                         # torch on the GPU in, the same out
    assert hard.is_cuda and np.array_equal(hard[:, 0].cpu().numpy(), g["attn_hard"].astype(np.float32))
    hard_np = b_mas(g["attn"][:, None], g["txt_lens"], g["mel_lens"])                 # numpy in, as the reference's caller passes it
    assert isinstance(hard_np, np.ndarray) and np.array_equal(hard_np[:, 0], g["attn_hard"].astype(np.float32))
    with pytest.raises(NotImplementedError):
        b_mas(attn, g["txt_lens"], g["mel_lens"], width=2)
    with pytest.raises(ValueError):
        enc(torch.from_numpy(g["mel"]).transpose(1, 2), torch.from_numpy(keys).transpose(1, 2), ~mask)   # not a prefix mask


def test_invariances_single_row_prior_tail_and_poisoned_workspace():
    g, h, keys, spk, prior, r = run_fixture("aligner_tiny_b3")
    want = ("dur", "attn_hard", "attn", "attn_logprob")
    # a B = 1 call with the batch's padding is its row of the batch, bit for bit
    for b in range(3):
        one = h.align(g["mel"][b:b + 1], keys[b:b + 1], spk[b:b + 1], g["txt_lens"][b:b + 1], g["mel_lens"][b:b + 1], prior[b:b + 1], want=want)
        for k in want:
            assert np.array_equal(one[k][0], r[k][b]), (k, b)
    # the padded tail of the prior.  What the reference's arithmetic makes of it is asked of the restatement, not assumed
    rng = np.random.Generator(np.random.PCG64(5))
    prior2 = prior.copy()
    for b, (n, m) in enumerate(zip(g["txt_lens"], g["mel_lens"])):
        prior2[b, m:, :] = rng.random(prior2[b, m:, :].shape)
        prior2[b, :, n:] = rng.random(prior2[b, :, n:].shape)
    P = ar.submodule_state(fixture_state(g))
    args = (P, g["mel"].transpose(0, 2, 1), keys.transpose(0, 2, 1), float(g["temperature"]), g["txt_lens"])
    ra, rl = ar.forward(*args, prior, spk)
    ra2, rl2 = ar.forward(*args, prior2, spk)
    ra64, rl64 = ar.forward(*args, prior2, spk, dtype=np.float64)
    same_a, same_l = ra == ra2, rl == rl2
    for b, (n, m) in enumerate(zip(g["txt_lens"], g["mel_lens"])):   # the restatement: frames < mel_len do not see the tail in attn, nor in logprob at keys < txt_len
        assert same_a[b, :m].all() and same_l[b, :m, :n].all()
        assert not same_l[b, :m, n:].all() if n < prior.shape[2] else True
    r2 = h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], prior2, want=want)
    assert np.array_equal(r2["attn"][same_a], r["attn"][same_a]) and np.array_equal(r2["attn_logprob"][same_l], r["attn_logprob"][same_l])
    assert np.array_equal(r2["dur"], r["dur"]) and np.array_equal(r2["attn_hard"], r["attn_hard"])
    full = np.full(3, prior.shape[1])   # where it does depend on the tail (every frame, every column), it follows the reference's arithmetic
    err_a, err_l = ar.valid_stats(ra2, ra64, g["txt_lens"], full), ar.valid_stats(rl2, rl64, g["txt_lens"], full, full_columns=True)
    check_bars("prior tail", r2["attn"], r2["attn_logprob"], ra64, rl64, err_a, err_l, g["txt_lens"], full)
    # a poisoned workspace changes nothing
    h.poison_workspace()
    r3 = h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], prior, want=want)
    for k in want:
        assert np.array_equal(r3[k], r[k]), k


def test_geometry_no_fixture_has_against_the_restatement():
    """hidden 128, n_mel 40, L = 33, T = 129 (no multiple of any tile), two rows of different lengths, with the prior."""
    H, M, B, L, T = 128, 40, 2, 33, 129
    txt_lens, mel_lens = np.array([33, 20], np.int64), np.array([129, 77], np.int64)
    state = sw.make_aligner_state(H, M, seed=91)
    rng = np.random.Generator(np.random.PCG64(17))
    ids = np.zeros((B, L), np.int64)
    for b in range(B):
        ids[b, :txt_lens[b]] = rng.integers(1, cfgmod.N_SYMBOLS + 1, txt_lens[b])
    mel = (rng.standard_normal((B, T, M)) * 2 - 4).astype(np.float32)
    for b in range(B):
        mel[b, mel_lens[b]:] = 0
    keys, spk = state["encoder.src_word_emb.weight"][ids], state["speaker_emb.weight"][np.array([1, 3])]
    prior = al.batch_prior(txt_lens, mel_lens, T, L)
    P = ar.submodule_state(state)
    args = (P, mel.transpose(0, 2, 1), keys.transpose(0, 2, 1), 5e-4, txt_lens, prior, spk)
    a32, l32 = ar.forward(*args)
    a64, l64 = ar.forward(*args, dtype=np.float64)
    h = al.Aligner(M, M, H, 5e-4, device=0)
    h.load_weights(packer.pack_aligner(state))
    r = h.align(mel, keys, spk, txt_lens, mel_lens, prior, want=("dur", "attn_hard", "attn", "attn_logprob"))
    check_bars("hidden 128 n_mel 40 L 33 T 129", r["attn"], r["attn_logprob"], a64, l64, ar.valid_stats(a32, a64, txt_lens, mel_lens),
               ar.valid_stats(l32, l64, txt_lens, mel_lens, full_columns=True), txt_lens, mel_lens)
    for b, n in enumerate(txt_lens):
        assert not r["attn"][b, :, n:].any()
    # the search on the library's own attn: the restatement's path on the same fp32 log map
    with np.errstate(divide="ignore"):
        loga = np.log(r["attn"])
    want = ar.b_mas(loga, txt_lens, mel_lens, log_map=True, search=ar.mas_rows)
    m = h.mas(loga, txt_lens, mel_lens, log_map=True)
    assert np.array_equal(m["attn_hard"], want) and np.array_equal(m["dur"].sum(1), mel_lens.astype(np.float32))


def test_long_rows_take_the_four_frame_attention_tile():
    """L = 700 at n_att 80: the scores of a 16-frame tile no longer fit 64 KB of LDS, so the attention pass runs 4 frames per workgroup (11 key
    tiles, the last one partial), and the search runs the workgroup form with three columns per thread.  Against the restatement."""
    H, M, B, L, T = 64, 80, 1, 700, 22
    txt_lens, mel_lens = np.array([700], np.int64), np.array([22], np.int64)
    state = sw.make_aligner_state(H, M, seed=92)
    rng = np.random.Generator(np.random.PCG64(23))
    ids = rng.integers(1, cfgmod.N_SYMBOLS + 1, (B, L))
    mel = (rng.standard_normal((B, T, M)) * 2 - 4).astype(np.float32)
    keys, spk = state["encoder.src_word_emb.weight"][ids], state["speaker_emb.weight"][np.array([2])]
    prior = rng.random((B, T, L)).astype(np.float32)     # (a beta-binomial prior over 700 phonemes underflows: any positive prior serves here)
    args = (ar.submodule_state(state), mel.transpose(0, 2, 1), keys.transpose(0, 2, 1), 5e-4, txt_lens, prior, spk)
    a32, l32 = ar.forward(*args)
    a64, l64 = ar.forward(*args, dtype=np.float64)
    h = al.Aligner(M, M, H, 5e-4, device=0)
    h.load_weights(packer.pack_aligner(state))
    r = h.align(mel, keys, spk, txt_lens, mel_lens, prior, want=("dur", "attn_hard", "attn", "attn_logprob"))
    check_bars("L 700 T 22", r["attn"], r["attn_logprob"], a64, l64, ar.valid_stats(a32, a64, txt_lens, mel_lens),
               ar.valid_stats(l32, l64, txt_lens, mel_lens, full_columns=True), txt_lens, mel_lens)
    with np.errstate(divide="ignore"):
        loga = np.log(r["attn"])
    assert np.array_equal(h.mas(loga, txt_lens, mel_lens, log_map=True)["attn_hard"], ar.b_mas(loga, txt_lens, mel_lens, log_map=True, search=ar.mas_rows))


def test_device_memory_is_three_maps_not_the_4d_tensor():
    """The structural claim: a handle fed from device memory holds about 3 [B, T, L] maps (attn, attn_logprob, attn_hard), one bit per cell
    of back-pointers and the projections' O(B (T + L) C) -- never the reference's [B, n_att, T, L] tensor."""
    import torch
    g = load_golden("aligner_full_b2")
    state, keys, spk, prior = fixture_inputs(g)
    H, M = int(g["hidden"]), int(g["n_mel"])
    h = al.Aligner(M, M, H, float(g["temperature"]), device=0)
    blob = packer.pack_aligner(state)
    h.load_weights(blob)
    B, T, L = g["attn"].shape
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    dur, hard = torch.empty((B, L), device="cuda"), torch.empty((B, T, L), device="cuda")
    h.align(dev(g["mel"]), dev(keys), dev(spk), g["txt_lens"], g["mel_lens"], dev(prior), out_dur=dur, out_hard=hard, want=())
    assert np.array_equal(dur.cpu().numpy(), g["dur"])
    maps = 3 * B * T * L * 4
    bits = B * T * ((L + 31) // 32) * 4
    proj = 4 * (B * L * (H + 2 * H + M) + B * T * (M + 2 * M) + B * (2 * H + M) + B * L + 2 * B)
    n_buffers = 20
    assert h.device_bytes() <= blob.size + maps + bits + proj + 256 * n_buffers
    assert h.device_bytes() - blob.size < B * M * T * L * 4 // 4    # (at this small shape the projections outweigh the maps; the line above is the tight bound)
    before = h.device_bytes()
    h.align(dev(g["mel"]), dev(keys), dev(spk), g["txt_lens"], g["mel_lens"], dev(prior), out_dur=dur, want=())
    assert h.device_bytes() == before          # steady state allocates nothing
