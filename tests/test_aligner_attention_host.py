"""CPU checks of what tests/test_gpu_aligner_attention.py relies on (tests/aligner_ref.py: attention64 and its bar, attention32_kernel_order;
tests/aligner_attn_cases.py): the float64 restatement against aligner_ref.forward's own lines, the instantiation each case takes, the
float32 restatement in the kernel's order under the bar at every case (its worst ratio printed), and every listed mutation failing the GPU
test's own check functions at the smallest case it exists in."""
import numpy as np
import pytest

import aligner_ref as ar
import aligner_attn_cases as ac

f32 = np.float32


def test_instantiations():
    for A, L, T in ac.SHAPES:
        assert ar.attn_frames_per_workgroup(L, A) == 16, (A, L)
    for A, L, T in ac.FOUR_FRAME_SHAPES:
        assert ar.attn_lds_bytes(16, L, A) > 64 * 1024 >= ar.attn_lds_bytes(4, L, A) and ar.attn_frames_per_workgroup(L, A) == 4
    assert ar.attn_frames_per_workgroup(2048, 128) is None
    assert {s[0] % 4 for s in ac.SHAPES} == {0, 1, 2, 3} and all(T <= 40 for _, _, T in ac.SHAPES + ac.FOUR_FRAME_SHAPES)
    got = {(m, p, t) for A, L, T, m, p, t in ac.general_cases() if (A, L, T) == ac.CROSS_SHAPE}
    assert len(got) == len(ac.LENS_MODES) * len(ac.PRIORS) * len(ac.TEMPS)


def test_attention64_is_the_references_formula():
    """aligner_ref.forward's lines from the squared distance on (the restatement the fixtures pin), in float64, on the same inputs."""
    A, L, T = ac.CROSS_SHAPE
    for lens_mode in ac.LENS_MODES:
        for prior_kind in ac.PRIORS:
            q, k, lens, prior = ac.general_inputs(A, L, T, lens_mode, prior_kind)
            a64, l64, ba, bl = ar.attention64(q, k, 5e-4, lens, prior)
            a = np.float64(f32(-5e-4)) * ((q.astype(np.float64)[:, :, None] - k.astype(np.float64)[:, None]) ** 2).sum(-1)
            if prior is not None:
                a = ar.log_softmax(a) + np.log(prior.astype(np.float64) + np.float64(f32(1e-8)))
            assert np.allclose(l64, a, rtol=1e-12, atol=1e-12)
            if lens is not None:
                for b in range(3):
                    a[b, :, int(lens[b]):] = -np.inf
            e = np.exp(a - a.max(-1, keepdims=True))
            assert np.allclose(a64, e / e.sum(-1, keepdims=True), rtol=1e-12, atol=1e-300)
            assert np.all(ba >= 0) and np.all(bl >= 0) and np.all(np.isfinite(ba)) and np.all(np.isfinite(bl))


def test_float32_restatement_stays_under_the_bar_at_every_case():
    worst = {"attn": 0.0, "attn_logprob": 0.0}
    for A, L, T, lens_mode, prior_kind, temp in ac.general_cases():
        q, k, lens, prior = ac.general_inputs(A, L, T, lens_mode, prior_kind)
        ref = ar.attention64(q, k, temp, lens, prior)
        a32, l32 = ar.attention32_kernel_order(q, k, temp, lens, prior)
        fails, fig = ac.check_general(a32, l32, ref, yard=(a32, l32))
        assert not fails and not ac.check_masked(a32, lens), (A, L, T, lens_mode, prior_kind, temp, fails)
        worst = {n: max(worst[n], fig[n]) for n in worst}
    print(f"[attention] float32 restatement in the kernel's order: worst error / bar attn {worst['attn']:.3f}, attn_logprob {worst['attn_logprob']:.3f}")
    assert max(worst.values()) < 1


def test_exact_tier_on_the_restatement():
    for A, L, T in ac.SHAPES + ac.FOUR_FRAME_SHAPES:
        for identical in (False, True):
            q, k = ac.exact_inputs(A, L, T, identical)
            for mode in ac.LENS_MODES:
                lens = ac.lens_of(mode, 3, L)
                a32, l32 = ar.attention32_kernel_order(q, k, ac.T_EXACT, lens, None)
                fails, nd = ac.check_exact(a32, l32, q, k, lens, identical)
                assert not fails and nd == 0, (A, L, T, identical, mode, fails)


# ---------------------------------------------------------------- mutations, through the GPU test's own check functions
def _general_fails(mut, A, L, T, lens_mode, prior_kind, temp=5e-4):
    q, k, lens, prior = ac.general_inputs(A, L, T, lens_mode, prior_kind)
    ref = ar.attention64(q, k, temp, lens, prior)
    a, l = ar.attention32_kernel_order(q, k, temp, lens, prior, mut=mut)
    return ac.check_general(a, l, ref)[0] + ac.check_masked(a, lens)


def _exact_fails(mut, A, L, T, lens_mode="ragged"):
    q, k = ac.exact_inputs(A, L, T)
    lens = ac.lens_of(lens_mode, 3, L)
    a, l = ar.attention32_kernel_order(q, k, ac.T_EXACT, lens, None, mut=mut)
    return ac.check_exact(a, l, q, k, lens)[0]


@pytest.mark.parametrize("A", [5, 6, 7])
def test_mutation_tail_channel_dropped(A):
    assert _exact_fails("tail", A, 65, 17) and _general_fails("tail", A, 65, 17, "full", "none")
    assert not _exact_fails(None, A, 65, 17)


def test_mutation_stale_keys_in_a_partial_key_tile():
    assert _exact_fails("stale", 8, 65, 17) and _exact_fails("stale", 8, 130, 17)
    assert not _exact_fails("stale", 8, 64, 17)               # no partial tile: the mutation does not exist there


def test_mutations_of_the_prior_the_mask_and_the_frame_tail():
    A, L, T = ac.CROSS_SHAPE
    assert _general_fails("prior_len", A, L, T, "ragged", "uniform") and _general_fails("prior_len", A, L, T, "one", "betabinom")
    assert not _general_fails("prior_len", A, L, T, "full", "uniform")      # len == L: provably the same computation
    assert _general_fails("softmax_L", A, L, T, "ragged", "none") and _exact_fails("softmax_L", A, L, T)
    assert _general_fails("mask+1", A, L, T, "ragged", "none") and _general_fails("mask+1", A, L, T, "one", "uniform") and _exact_fails("mask+1", A, L, T)
    assert _general_fails("no_eps", A, L, T, "ragged", "betabinom")         # the padded prior is 0 past a row's phonemes: log 0
    assert _general_fails("no_eps", A, L, T, "absent", "betabinom")         # and the beta-binomial tails lie far below 1e-8
    assert _general_fails("skip_last", A, L, T, "full", "none") and _exact_fails("skip_last", A, L, T) and _exact_fails("skip_last", A, L, 1)
    assert not _exact_fails("skip_last", A, L, 16)            # a whole tile: the mutation does not exist there
