"""CPU checks of tests/aligner_tie_cases.py: the maps of tests/test_gpu_aligner_ties.py discriminate.
  - the switchable restatement equals aligner_ref.mas_rows (and the plain two-loop mas_loops) on every case;
  - `>` in place of `>=` changes the path at every case that has an alternative path at all (L = 1 has one column and T = 1 has one frame:
    provably none), counted per width over its frame counts and maps;
  - taking the left neighbour of a lane's first column as -inf changes the path at L = 65 (two columns per lane) and L = 129 (four), and at
    every other width those forms serve;
  - the workspace cases are past the LDS budget of their form, and the sums of every map are exact in float32."""
import numpy as np
import pytest

import aligner_ref as ar
import aligner_tie_cases as tc


def _cases(L):
    for T in tc.frames_of(L):
        il, ol = tc.lens_of(T, L)
        for kind in tc.KINDS:
            yield kind, T, tc.tie_map(kind, 3, T, L), il, ol


@pytest.mark.parametrize("L", tc.WIDTHS)
def test_strict_comparison_changes_the_path(L):
    changed = {}
    for kind, T, a, il, ol in _cases(L):
        want = tc.want_of(kind, a, il, ol)
        assert np.array_equal(want, ar.b_mas(a, il, ol, log_map=kind != "prob01", search=ar.mas_rows))
        if T <= 17 and L <= 33:
            assert np.array_equal(want, ar.b_mas(a, il, ol, log_map=kind != "prob01", search=ar.mas_loops))
        assert np.array_equal(want.sum((1, 2)), np.maximum(ol, 1) + (il > ol))          # one mark per frame, and the closing opt[0, 0]
        changed[kind, T] = not np.array_equal(want, tc.want_of(kind, a, il, ol, strict=True))
    if L == 1:
        assert not any(changed.values())          # one column: no other path exists
        return
    assert not any(v for (k, T), v in changed.items() if T == 1)      # one frame: no step is taken
    tall = L + 9
    for kind in tc.KINDS:
        assert changed[kind, tall], (kind, L)                          # finite ties on the path
        if L >= 31:
            assert all(changed[kind, T] for T in tc.FRAMES if T >= 2), (kind, L, changed)     # -inf ties down the diagonal


@pytest.mark.parametrize("L", [w for w in tc.WIDTHS if tc.form_of(w) > 1])
def test_a_lost_left_neighbour_changes_the_path(L):
    """The column a lane receives from the lane before it (one shuffle per frame): lost, the path differs on the finite-tie map."""
    c = tc.form_of(L)
    assert (L, c) not in ((65, 4), (129, 2)) and c == (2 if L <= 128 else 4)
    T = L + 9
    il, ol = tc.lens_of(T, L)
    a = tc.tie_map("log4", 3, T, L)
    assert not np.array_equal(tc.want_of("log4", a, il, ol), tc.want_of("log4", a, il, ol, blind=c))


def test_workspace_cases_and_exact_sums():
    budget = 40 * 1024                                   # aligner.hip: MAS_LDS_BUDGET, over the [L] rows (one, or three in the workgroup form) + the bits
    for B, T, L in tc.WORKSPACE_CASES:
        assert (1 if L <= 256 else 3) * L * 4 + T * ((L + 31) // 32) * 4 > budget
        a = tc.tie_map("log4", B, T, L)
        il, ol = np.full(B, L, np.int64), np.full(B, T, np.int64)
        assert not np.array_equal(tc.want_of("log4", a, il, ol), tc.want_of("log4", a, il, ol, strict=True))
    assert 3 * 5200 < 2 ** 24                            # every partial sum of a log4 map is an integer below 2^24: exact in float32
    assert [tc.form_of(w) for w in (64, 65, 128, 129, 256, 257)] == [1, 2, 2, 4, 4, 0]
