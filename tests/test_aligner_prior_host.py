"""The generated beta-binomial prior, the parts that need no GPU: the float64 restatement of the header's formula
(tests/aligner_prior_ref.py) against the host path (aligner.batch_prior: scipy's betabinom.pmf, which equals the reference's stored
priors bit for bit) under the criterion the device is held to, the mutations that criterion must catch, and the refusals of
e2ealign_prior / e2ealign_forward_bb / e2ealign_align_bb, which happen before a device is opened."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
import aligner_prior_cases as pc
import aligner_prior_ref as pr
from e2e_tts_amd import aligner as al


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_align_hash() != g.align_hash() or g.built_align_hash(g.AL_TEST_LIB) != g.align_hash():
        g.build()
    return al.load_library()


def test_the_host_path_is_the_references_stored_prior():
    for name in ("aligner_tiny_b3", "aligner_tiny_wide_b1"):
        g = load_golden(name)
        T, L = g["mel"].shape[1], g["ids"].shape[1]
        want = al.batch_prior(g["txt_lens"], g["mel_lens"], T, L)
        assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), g["prior"].view(np.uint32))
    P, M, T, L, s = pc.case("ragged")          # the ragged case IS the first fixture's batch
    g = load_golden("aligner_tiny_b3")
    assert np.array_equal(P, g["txt_lens"]) and np.array_equal(M, g["mel_lens"]) and np.array_equal(pc.want("ragged"), g["prior"])


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_meets_the_criterion(name):
    P, M, T, L, s = pc.case(name)
    got = pr.batch64(P, M, T, L, s)
    fails, fig = pr.check_prior(got, pc.want(name), P, M)
    print(f"[prior restatement] {name}: {fig['normal']} normal-range elements, share differing {fig['share']:.2e}, max ulp {fig['max_ulp']}")
    assert not fails, fails
    assert fig["share"] == 0.0          # measured: the restatement and scipy agree on every element of these shapes


def test_criterion_on_its_own_edges():
    P, M = np.array([3], np.int64), np.array([2], np.int64)
    want = al.batch_prior(P, M, 3, 4)
    assert not pr.check_prior(want.copy(), want, P, M)[0]
    for at in [(0, 2, 0), (0, 0, 3)]:            # a padded frame, a padded column
        bad = want.copy()
        bad[at] = np.float32(1e-45)
        assert pr.check_prior(bad, want, P, M)[0]
    two = want.copy()
    two.view(np.uint32)[0, 0, 0] += 2
    assert pr.check_prior(two, want, P, M)[0]
    one = want.copy()
    one.view(np.uint32)[0, 0, 0] += 1            # 1 ulp is inside the bar, but 1 of 6 elements is above the share
    fails, fig = pr.check_prior(one, want, P, M)
    assert fig["max_ulp"] == 1 and len(fails) == 1 and "differ" in fails[0]
    nan = want.copy()
    nan[0, 0, 0] = np.nan
    assert pr.check_prior(nan, want, P, M)[0]
    # below the normal range: the subnormal, 0 and anything up to 2^-126 pass; more does not
    P, M = np.array([700], np.int64), np.array([22], np.int64)
    want = al.batch_prior(P, M, 22, 700)
    small = want < pr.F32_MIN_NORMAL
    assert small.any() and (want >= pr.F32_MIN_NORMAL).any()
    flushed = np.where(small, np.float32(0), want)
    assert not pr.check_prior(flushed, want, P, M)[0]
    lifted = np.where(small, np.float32(2.0 ** -125), want)
    assert pr.check_prior(lifted, want, P, M)[0]


@pytest.mark.parametrize("mutation", pr.MUTATIONS)
def test_every_mutation_fails_the_criterion(mutation):
    s = 2.5 if mutation == "scaling_alpha_only" else 1.0
    caught = []
    for P, M in ((7, 3), (12, 70)):
        pl, ml = np.array([P], np.int64), np.array([M], np.int64)
        T, L = M, P + 1 if mutation == "outcome_P_stored" else P          # (a column for outcome P to land in)
        want = al.batch_prior(pl, ml, T, L, s)
        assert not pr.check_prior(pr.batch64(pl, ml, T, L, s), want, pl, ml)[0]
        fails, fig = pr.check_prior(pr.batch64(pl, ml, T, L, s, mutation), want, pl, ml)
        print(f"[prior mutation] {mutation} at ({P}, {M}): {fails or 'PASSES'}")
        caught.append(bool(fails))
    assert any(caught)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host arrays, no GPU needed: nothing is allocated (device_bytes stays 0) and the handle stays usable."""
    h = C.c_void_p()
    assert lib.e2ealign_create(0, 80, 80, 64, 5e-4, C.byref(h)) == al.E_OK
    B, T, L = 2, 6, 5
    out = np.full((B, T, L), 7.0, np.float32)
    tl, ml = np.array([5, 3], np.int64), np.array([6, 4], np.int64)
    mel, keys = np.zeros((B, T, 80), np.float32), np.zeros((B, L, 64), np.float32)
    q, k = np.zeros((B, T, 80), np.float32), np.zeros((B, L, 80), np.float32)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def prior(tl=tl, ml=ml, B=B, T=T, L=L, s=1.0, out=out):
        return lib.e2ealign_prior(h, p(tl), p(ml), B, T, L, s, p(out))

    def forward_bb(tl=tl, ml=ml, B=B, T=T, L=L, s=1.0):
        return lib.e2ealign_forward_bb(h, p(mel), p(keys), None, p(tl), p(ml), s, B, T, L, None, None)

    def align_bb(tl=tl, ml=ml, B=B, T=T, L=L, s=1.0):
        return lib.e2ealign_align_bb(h, p(mel), p(keys), None, p(tl), p(ml), s, B, T, L, None, None, None, None)

    def attention_bb(tl=tl, ml=ml, B=B, T=T, L=L, s=1.0):
        return lib.e2ealign_debug_attention_bb(h, p(q), p(k), p(tl), p(ml), s, B, T, L, None, None)

    for call in (prior, forward_bb, align_bb, attention_bb):
        assert call(tl=None) == al.E_INVAL and b"NULL" in lib.e2ealign_last_error(h)
        assert call(ml=None) == al.E_INVAL and b"NULL" in lib.e2ealign_last_error(h)
        assert call(tl=np.array([6, 3], np.int64)) == al.E_INVAL and b"txt_lens[0] = 6" in lib.e2ealign_last_error(h)
        assert call(tl=np.array([5, 0], np.int64)) == al.E_INVAL and b"txt_lens[1] = 0" in lib.e2ealign_last_error(h)
        assert call(ml=np.array([6, 7], np.int64)) == al.E_INVAL and b"mel_lens[1] = 7" in lib.e2ealign_last_error(h)
        assert call(ml=np.array([-1, 4], np.int64)) == al.E_INVAL
        for s in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), al.MAX_PRIOR_SCALING * 1.0000001, 1e300):
            assert call(s=s) == al.E_INVAL and b"scaling" in lib.e2ealign_last_error(h), s
        assert call(B=0) == al.E_INVAL and call(B=al.MAX_B + 1) == al.E_INVAL
        assert call(T=0) == al.E_INVAL and call(T=-3) == al.E_INVAL and call(T=1 << 28) == al.E_INVAL
        assert call(L=0) == al.E_INVAL and call(L=al.MAX_L + 1) == al.E_INVAL
    assert prior(out=None) == al.E_INVAL and b"prior_out" in lib.e2ealign_last_error(h)
    # valid arguments, no weights: a matter of call order, found after the arguments were checked
    assert forward_bb() == al.E_STATE and align_bb() == al.E_STATE
    assert forward_bb(s=al.MAX_PRIOR_SCALING) == al.E_STATE
    assert lib.e2ealign_device_bytes(h) == 0 and (out == 7.0).all()
    assert lib.e2ealign_sync(h) == al.E_OK
    assert prior(s=0.0) == al.E_INVAL and b"scaling" in lib.e2ealign_last_error(h)      # still usable: the same refusal
    lib.e2ealign_destroy(h)
    a = al.Aligner(80, 80, 64, 5e-4)
    with pytest.raises(ValueError, match="device"):
        a.forward(mel, keys, None, tl, "host")
    with pytest.raises(ValueError, match="mel_lens"):
        a.forward(mel, keys, None, tl, "device")
    with pytest.raises(ValueError, match="scaling"):
        a.prior(tl, ml, T, L, scaling_factor=0.0)
    with pytest.raises(ValueError, match="scaling"):
        a.align(mel, keys, None, tl, ml, "device", prior_scaling=-2.0)
