"""GPU tests (-m gpu) of the beta-binomial attention prior generated on the device (include/e2etts_align.h: e2ealign_prior,
e2ealign_forward_bb / e2ealign_align_bb, and e2ealign_debug_attention_bb of the test build).

Three claims.  e2ealign_prior's tensor meets ``check_prior`` (tests/aligner_prior_ref.py: 1 fp32 ulp in the normal range, at most 0.1 % of
the elements differing at all, [0, 2^-126] below it, exact zeros in the padding) against the host path, scipy's betabinom.pmf, on
every case of tests/aligner_prior_cases.py.  The generated-prior form of the attention pass gives the SAME BITS as the given-prior form
fed that tensor: both kernels call one out-of-line function per cell.  And the generated path holds no [B, T, L] prior in device memory.
Measured figures: profiles/aligner/README.md."""
import numpy as np
import pytest

from conftest import load_golden
import aligner_prior_cases as pc
import aligner_prior_ref as pr
import aligner_ref as ar
from aligner_cases import fixture_inputs
from e2e_tts_amd import aligner as al, packer
from test_gpu_aligner import check_bars
from test_gpu_kernels import record

pytestmark = pytest.mark.gpu

_H = {}
WANT = ("dur", "attn_hard", "attn", "attn_logprob")


def bare(A=8, temperature=5e-4):
    """A handle without weights: all that e2ealign_prior and the attention pass alone need."""
    if (A, temperature) not in _H:
        _H[A, temperature] = al.Aligner(4, A, 4, temperature, device=0)
    return _H[A, temperature]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_prior_meets_the_criterion_on_every_case(name):
    P, M, T, L, s = pc.case(name)
    got = bare().prior(P, M, T, L, s)
    fails, fig = pr.check_prior(got, pc.want(name), P, M)
    print(f"[prior] {name}: {fig['normal']} normal-range elements, share differing {fig['share']:.3e}, max ulp {fig['max_ulp']}")
    record("aligner_prior", case=name, **fig)
    assert not fails, fails


def test_prior_output_pointers_single_rows_and_a_poisoned_workspace():
    import torch
    P, M, T, L, s = pc.case("ragged_padded")
    h = bare()
    host = h.prior(P, M, T, L, s)
    dev = torch.full((len(P), T, L), float("nan"), device="cuda")
    assert h.prior(P, M, T, L, s, out=dev) is dev
    assert np.array_equal(bits(dev.cpu().numpy()), bits(host))                       # host and device output pointers
    dev_lens = h.prior(torch.from_numpy(P).cuda(), torch.from_numpy(M).cuda(), T, L, s)
    assert np.array_equal(bits(dev_lens), bits(host))                                 # length arrays in device memory
    for b in range(len(P)):                                                           # B = 1 is its row of the batch, bit for bit
        assert np.array_equal(bits(h.prior(P[b:b + 1], M[b:b + 1], T, L, s)[0]), bits(host[b])), b
    h.poison_workspace()
    assert np.array_equal(bits(h.prior(P, M, T, L, s)), bits(host))
    into = np.full((len(P), T, L), np.nan, np.float32)
    assert h.prior(P, M, T, L, s, out=into) is into and np.array_equal(bits(into), bits(host))
    with pytest.raises(ValueError):
        h.prior(P, M, T, L - 60, s)                                                   # txt_lens[0] > L: refused, and the handle goes on
    assert np.array_equal(bits(h.prior(P, M, T, L, s)), bits(host))


# (n_att, L, T, txt_lens, mel_lens, scaling): L in {12, 64, 65, 130}, T no multiple of 16 or of 4, txt_lens < L and mel_lens < T in one batch
ATTENTION_CASES = [(8, 12, 70, (12, 7, 1), (70, 33, 5), 1.0),
                   (6, 64, 17, (64, 40, 64), (17, 17, 9), 1.0),
                   (80, 65, 33, (65, 1, 33), (33, 20, 1), 0.5),
                   (5, 130, 21, (130, 77, 129), (21, 5, 16), 2.5),
                   (80, 700, 22, (700,), (22,), 1.0),                 # the shape of test_long_rows_take_the_four_frame_attention_tile
                   (127, 400, 6, (400, 399, 13), (6, 5, 2), 1.0)]     # the 4-frame tile with both kinds of padding, T = 6


@pytest.mark.parametrize("A,L,T,tl,ml,s", ATTENTION_CASES)
def test_generated_attention_equals_the_given_prior_form_bit_for_bit(A, L, T, tl, ml, s):
    assert ar.attn_frames_per_workgroup(L, A) == (4 if L >= 400 else 16)
    B = len(tl)
    rng = np.random.Generator(np.random.PCG64(A * 1000 + L))
    q, k = rng.standard_normal((B, T, A)).astype(np.float32), rng.standard_normal((B, L, A)).astype(np.float32)
    tl, ml = np.asarray(tl, np.int64), np.asarray(ml, np.int64)
    h = bare(A)
    prior = h.prior(tl, ml, T, L, s)
    assert prior.any() and not prior[0, ml[0]:].any() and not prior[-1, :, tl[-1]:].any()
    given = h.debug_attention(q, k, prior, tl)
    h.poison_workspace()
    gen = h.debug_attention_bb(q, k, tl, ml, s)
    for name in ("attn", "attn_logprob"):
        assert not np.isnan(gen[name]).any()
        nd = int((bits(gen[name]) != bits(given[name])).sum())
        assert nd == 0, f"{name}: {nd} of {gen[name].size} elements differ"
    host = ar.attention32_kernel_order(q, k, 5e-4, tl, al.batch_prior(tl, ml, T, L, s))   # and the prior is the right one, not merely the same one
    assert np.allclose(gen["attn"], host[0], atol=1e-5)


@pytest.mark.parametrize("name", ["aligner_tiny_b3", "aligner_tiny_wide_b1", "aligner_full_b2"])
def test_align_bb_on_the_fixtures(name):
    g = load_golden(name)
    state, keys, spk, _ = fixture_inputs(g)
    h = al.Aligner(int(g["n_mel"]), int(g["n_mel"]), int(g["hidden"]), float(g["temperature"]), device=0)
    h.load_weights(packer.pack_aligner(state))
    B, T, L = g["attn"].shape
    r = h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], "device", want=WANT)
    assert np.array_equal(r["dur"], g["dur"]) and np.array_equal(r["attn_hard"], g["attn_hard"].astype(np.float32))
    check_bars(name + " generated prior", r["attn"], r["attn_logprob"], g["attn64"], g["attn_logprob64"], g["ref_err_attn"], g["ref_err_logprob"],
               g["txt_lens"], g["mel_lens"])
    given = h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], h.prior(g["txt_lens"], g["mel_lens"], T, L), want=WANT)
    for k in WANT:
        assert np.array_equal(bits(r[k]), bits(given[k])), k
    f = h.forward(g["mel"], keys, spk, g["txt_lens"], "device", mel_lens=g["mel_lens"])
    assert np.array_equal(bits(f["attn"]), bits(r["attn"])) and np.array_equal(bits(f["attn_logprob"]), bits(r["attn_logprob"]))
    m = h.mas(None, g["txt_lens"], g["mel_lens"], B=B, T=T, L=L)                      # the maps of forward_bb are resident like any other's
    assert np.array_equal(m["dur"], g["dur"])


def test_the_generated_path_holds_no_prior_buffer():
    g = load_golden("aligner_full_b2")
    state, keys, spk, _ = fixture_inputs(g)
    blob = packer.pack_aligner(state)
    B, T, L = g["attn"].shape
    held = []
    for prior in (None, "device"):
        h = al.Aligner(int(g["n_mel"]), int(g["n_mel"]), int(g["hidden"]), float(g["temperature"]), device=0)
        h.load_weights(blob)
        h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], prior, want=WANT)
        held.append(h.device_bytes())
        h.close()
    assert held[0] == held[1], held
    h = al.Aligner(int(g["n_mel"]), int(g["n_mel"]), int(g["hidden"]), float(g["temperature"]), device=0)
    h.load_weights(blob)
    h.align(g["mel"], keys, spk, g["txt_lens"], g["mel_lens"], np.ones((B, T, L), np.float32), want=WANT)
    assert h.device_bytes() >= held[1] + B * T * L * 4          # what a prior given in host memory holds on top
