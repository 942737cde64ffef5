"""Host side of the vocoder-bias denoiser (reference e2e_tts/models/vocoder/denoiser.py: STFT :55-153, Denoiser :156-186).

``stft_bases`` builds the two windowed bases with the numpy / scipy calls the reference's ``STFT.__init__`` makes (``np.fft.fft`` of
the identity, ``np.linalg.pinv``, ``scipy.signal.get_window``), in the reference's own buffer layout, which is what
``e2etts_denoiser_load`` takes.  Everything that touches samples runs in the engine (csrc/denoiser.hip); there is no CPU path here.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

N_OVERLAPS = (2, 4, 8)   # filter_length / hop the engine serves
MAX_HOP = 1024   # csrc/denoiser.hip keeps one spectrum row (filter_length + 2 floats) in LDS: 32 KiB at hop 1024 x 8


def check_geometry(filter_length: int, hop: int) -> int:
    """The geometries e2etts_denoiser_load accepts; returns n_overlap, raises ValueError with the numbers otherwise."""
    filter_length, hop = int(filter_length), int(hop)
    if filter_length <= 0 or hop <= 0 or filter_length % hop:
        raise ValueError(f"denoiser: filter_length {filter_length} is not hop {hop} x n_overlap")
    n_overlap = filter_length // hop
    if n_overlap not in N_OVERLAPS:
        raise ValueError(f"denoiser: n_overlap = filter_length / hop = {filter_length} / {hop} = {n_overlap}, served: {N_OVERLAPS}")
    if hop % 32 or hop > MAX_HOP:
        raise ValueError(f"denoiser: hop {hop} must be a multiple of 32, at most {MAX_HOP}")
    return n_overlap


def check_lengths(n_valid, n: int, hop: int) -> np.ndarray:
    """Valid samples per row as e2etts_denoise takes them: int64, each in [0, n] and a multiple of hop (vocoder output always is)."""
    nv = np.ascontiguousarray(np.asarray(n_valid, dtype=np.int64).reshape(-1))
    bad = [(b, int(v)) for b, v in enumerate(nv) if v < 0 or v > n or v % hop]
    if bad:
        raise ValueError(f"denoiser: valid lengths (row, samples) {bad} must lie in [0, {n}] and be multiples of the hop {hop}")
    return nv


def stream_delay_frames(filter_length: int, hop: int, hop_length: int) -> int:
    """Mel frames of context a denoised vocoder stream keeps on each side beyond the vocoder's halo (``*delay_frames_out`` of
    e2etts_vocoder_stream_begin_denoised).  A denoised sample depends on the input samples strictly closer than filter_length - hop: every
    frame that covers it, and every sample those frames cover; hop_length must be a multiple of hop, so that windows start on the frame grid."""
    filter_length, hop, hop_length = int(filter_length), int(hop), int(hop_length)
    check_geometry(filter_length, hop)
    if hop_length <= 0 or hop_length % hop:
        raise ValueError(f"denoiser: hop {hop} does not divide the vocoder's hop_length {hop_length}")
    return -(-(filter_length - hop) // hop_length)


def centre_pad(x: np.ndarray, size: int) -> np.ndarray:
    """Zero-pad to `size` with the data in the middle (the extra sample of an odd difference goes to the right)."""
    if len(x) > size:
        raise ValueError(f"denoiser: win_length {len(x)} exceeds filter_length {size}")
    left = (size - len(x)) // 2
    return np.pad(x, (left, size - len(x) - left))


def stft_bases(filter_length: int, hop: int, win_length: int, window: str = "hann") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (forward_basis, inverse_basis) float32 [filter_length + 2, filter_length] -- real rows of the first filter_length / 2 + 1 DFT
    vectors, then their imaginary rows, as ``STFT.forward_basis`` / ``inverse_basis`` squeezed (V/denoiser.py:65-88) -- and the squared,
    centre-padded window [filter_length] in float64 (the sum-square envelope's, :43-46).  Any window ``scipy.signal.get_window`` names;
    ``win_length < filter_length`` is centre-padded."""
    from scipy.signal import get_window
    check_geometry(filter_length, hop)
    N = int(filter_length)
    dft = np.fft.fft(np.eye(N))
    bins = N // 2 + 1
    basis = np.vstack([dft[:bins].real, dft[:bins].imag])
    win = centre_pad(get_window(window, int(win_length), fftbins=True), N)
    win32 = win.astype(np.float32)
    fwd = basis.astype(np.float32) * win32
    inv = np.linalg.pinv((N / hop) * basis).T.astype(np.float32) * win32
    return np.ascontiguousarray(fwd), np.ascontiguousarray(inv), win ** 2


def engine_window(win_sq: np.ndarray, filter_length: int, win_length: int, window: str):
    """What e2etts_denoiser_load gets for the envelope: None for the periodic Hann of filter_length points (the engine forms it in
    float64, as the reference's envelope does), else the squared window rounded to float32."""
    if window == "hann" and int(win_length) == int(filter_length):
        return None
    return np.ascontiguousarray(win_sq, dtype=np.float32)
