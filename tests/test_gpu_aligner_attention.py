"""GPU tests (-m gpu) of aln_attn_kernel ALONE, through e2ealign_debug_attention of the test build (Aligner.debug_attention): the caller's
q [B, T, n_att] and k [B, L, n_att] go straight into the attention pass, launched by the same function that e2ealign_forward uses, so no
convolution stands between the inputs and the kernel and n_att need not equal n_mel.  Shapes, tiers and check functions:
tests/aligner_attn_cases.py; restatements and the derivation of the per-element bar: tests/aligner_ref.py (attention64).  No weights are
loaded; every handle is created with the n_att under test and n_mel = n_text = 4."""
import time

import numpy as np
import pytest

import aligner_ref as ar
import aligner_attn_cases as ac
from e2e_tts_amd import aligner as al
from test_gpu_kernels import record

pytestmark = pytest.mark.gpu

_H = {}
_T0 = time.time()
_worst = {"attn": 0.0, "attn_logprob": 0.0, "attn_agg": 0.0, "attn_logprob_agg": 0.0}
_count = {"exact": [0, 0, 0], "general": [0, 0]}


def handle(A, temperature):
    key = (A, float(temperature))
    if key not in _H:
        _H[key] = al.Aligner(4, A, 4, temperature, device=0)
    return _H[key]


@pytest.mark.parametrize("A,L,T", ac.SHAPES + ac.FOUR_FRAME_SHAPES)
def test_exact_tier(A, L, T):
    """attn_logprob bit for bit on every column, attn exactly 0 on masked keys and exactly fl(1 / len) on identical keys, at every txt_lens
    mode; the handle's workspace poisoned first, so nothing stale can pass for a value."""
    assert ar.attn_frames_per_workgroup(L, A) == (4 if (A, L, T) in ac.FOUR_FRAME_SHAPES else 16)
    h = handle(A, ac.T_EXACT)
    for identical in (False, True):
        q, k = ac.exact_inputs(A, L, T, identical)
        for mode in ac.LENS_MODES:
            lens = ac.lens_of(mode, 3, L)
            h.poison_workspace()
            r = h.debug_attention(q, k, None, lens)
            fails, nd = ac.check_exact(r["attn"], r["attn_logprob"], q, k, lens, identical)
            _count["exact"][0] += 1
            _count["exact"][1] += r["attn_logprob"].size
            _count["exact"][2] += nd
            assert not fails, (A, L, T, identical, mode, fails)


@pytest.mark.parametrize("A,L,T,lens_mode,prior_kind,temp", ac.general_cases())
def test_general_tier(A, L, T, lens_mode, prior_kind, temp):
    q, k, lens, prior = ac.general_inputs(A, L, T, lens_mode, prior_kind)
    ref = ar.attention64(q, k, temp, lens, prior)
    yard = ar.attention32_kernel_order(q, k, temp, lens, prior)
    h = handle(A, temp)
    h.poison_workspace()
    r = h.debug_attention(q, k, prior, lens)
    fails, fig = ac.check_general(r["attn"], r["attn_logprob"], ref, yard)
    fails += ac.check_masked(r["attn"], lens)
    for name, v in fig.items():
        _worst[name] = max(_worst[name], v)
    _count["general"][0] += 1
    _count["general"][1] += 2 * r["attn"].size
    print(f"[attention] A {A} L {L} T {T} {lens_mode} {prior_kind} t {temp:g}: {fig}")
    assert not fails, fails


def test_figures_and_wall_time():
    print(f"[attention] exact tier: {_count['exact'][0]} launches, {_count['exact'][1]} attn_logprob elements, {_count['exact'][2]} differing; "
          f"general tier: {_count['general'][0]} launches, {_count['general'][1]} elements; worst error / bar attn {_worst['attn']:.3f}, "
          f"attn_logprob {_worst['attn_logprob']:.3f}; worst mean deviation / the float32 restatement's: attn {_worst['attn_agg']:.3f}, "
          f"attn_logprob {_worst['attn_logprob_agg']:.3f}; wall time {time.time() - _T0:.1f} s")
    record("aligner_attention", exact_launches=_count["exact"][0], exact_elements=_count["exact"][1], exact_differing=_count["exact"][2],
           general_launches=_count["general"][0], general_elements=_count["general"][1], seconds=time.time() - _T0, **_worst)
