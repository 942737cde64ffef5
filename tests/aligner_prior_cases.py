"""The cases of the generated beta-binomial prior that tests/test_aligner_prior_host.py (the float64 restatement, on the CPU) and
tests/test_gpu_aligner_prior.py (e2ealign_prior, on the GPU) share, and the host path's tensor of each -- computed once, left unchanged."""
from __future__ import annotations

import numpy as np

from e2e_tts_amd import aligner as al

# name -> (txt_lens P, mel_lens M, T, L, scaling)
CASES = {}
for _P, _M in [(1, 1), (1, 5), (5, 1), (7, 3), (12, 70), (64, 64), (65, 129), (70, 150),
               (700, 22), (2048, 24),        # rows for the 4-frame attention tile and the widest row: nearly every value underflows
               (33, 4000)]:                  # the largest log-gamma arguments
    CASES[f"{_P}x{_M}"] = ([_P], [_M], _M, _P, 1.0)
CASES["ragged"] = ([12, 7, 1], [70, 33, 5], 70, 12, 1.0)          # the fixture batch aligner_tiny_b3
CASES["ragged_padded"] = ([12, 7, 1], [70, 33, 5], 81, 70, 1.0)   # the same rows padded further
CASES["40x300_s0.5"] = ([40], [300], 300, 40, 0.5)
CASES["40x300_s2.5"] = ([40], [300], 300, 40, 2.5)

_WANT = {}


def case(name):
    """(txt_lens int64, mel_lens int64, T, L, scaling) of a case."""
    P, M, T, L, s = CASES[name]
    return np.asarray(P, np.int64), np.asarray(M, np.int64), T, L, s


def want(name):
    """aligner.batch_prior (scipy's betabinom.pmf, the reference's path) on the case: [B, T, L] float32, read-only."""
    if name not in _WANT:
        P, M, T, L, s = case(name)
        w = al.batch_prior(P, M, T, L, s)
        w.setflags(write=False)
        _WANT[name] = w
    return _WANT[name]
