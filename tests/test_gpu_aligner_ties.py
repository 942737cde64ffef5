"""GPU tests (-m gpu) of the monotonic search under ties, through Aligner.mas: every kernel form (1, 2 and 4 columns per lane of the
one-wavefront kernel, the workgroup kernel at two and three columns per thread), every back-pointer word boundary and both placements of
the back-pointer bits, on the maps of tests/aligner_tie_cases.py, whose partial sums are exact and on which ties are the norm.  attn_hard
and dur are judged bit for bit against aligner_ref.mas_rows (the reference's `>=`: a tie, -inf ties included, takes the diagonal).
tests/test_aligner_ties_host.py shows on the CPU that these cases tell `>` from `>=` and a lost left neighbour from a delivered one."""
import time

import numpy as np
import pytest

import aligner_ref as ar
import aligner_tie_cases as tc
from e2e_tts_amd import aligner as al

pytestmark = pytest.mark.gpu

_H = {}
_T0 = time.time()
_count = [0, 0]


def handle():
    if "h" not in _H:
        _H["h"] = al.Aligner(4, 1, 4, 1.0, device=0)
    return _H["h"]


def judge(kind, a, il, ol):
    log_map = kind != "prob01"
    want = ar.b_mas(a, il, ol, log_map=log_map, search=ar.mas_rows)
    r = handle().mas(a, il, ol, log_map=log_map)
    _count[0] += 1
    _count[1] += want.size
    assert np.array_equal(r["attn_hard"], want), (kind, a.shape, int((r["attn_hard"] != want).sum()))
    assert np.array_equal(r["dur"], want.sum(1))


@pytest.mark.parametrize("L", tc.WIDTHS)
def test_search_under_ties(L):
    """B = 3 (a whole row, a row ragged in both lengths, a row with fewer frames than phonemes) at every frame count, on all three maps."""
    for T in tc.frames_of(L):
        il, ol = tc.lens_of(T, L)
        for kind in tc.KINDS:
            judge(kind, tc.tie_map(kind, 3, T, L), il, ol)


@pytest.mark.parametrize("B,T,L", tc.WORKSPACE_CASES)
def test_search_under_ties_with_the_bits_in_the_workspace(B, T, L):
    a = tc.tie_map("log4", B, T, L)
    judge("log4", a, np.full(B, L, np.int64), np.full(B, T, np.int64))


def test_wall_time():
    print(f"[aligner ties] {_count[0]} searches, {_count[1]} cells compared, 0 differing; wall time {time.time() - _T0:.1f} s")
