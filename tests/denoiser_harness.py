"""ctypes binding of the e2ekt_* entry points of tests/csrc/denoiser_harness.hip (libe2etts_kernels_test.so): the seven launch wrappers of
csrc/denoiser.hip.  Device buffers are passed as `torch.Tensor.data_ptr()` integers (or None); every entry returns the wrapper's message
(None = launched).  A wrapper that refuses returns before it launches, so the refusals work without a GPU (the pointers are never
dereferenced: pass any non-zero, suitably aligned integer for 'present')."""
from __future__ import annotations

import ctypes as C

from kernel_harness import LIB_PATH, F, I, LL, P, S, _msg   # noqa: F401

LLONG_MAX = 2 ** 63 - 1
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    import os
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py`")
    import torch  # noqa: F401  -- first, so that the process has ONE HIP runtime (see e2e_tts_amd/_lib.load_library)
    lib = C.CDLL(LIB_PATH)

    def bind(name, args):
        f = getattr(lib, name)
        f.restype = S
        f.argtypes = args

    bind("e2ekt_denoiser_version", [])
    bind("e2ekt_stft_pad", [P, LL, P, P, I, I, I, I, P])
    bind("e2ekt_spectral_subtract", [P, P, P, I, I, I, I, I, F, P])
    bind("e2ekt_bias_frame", [P, P, I, P])
    bind("e2ekt_ola_norm", [P, P, LL, P, P, P, P, P, I, LL, I, I, I, P])
    bind("e2ekt_stft_pad_stream", [P, LL, P, I, LL, I, I, I, I, I, P])
    bind("e2ekt_fill_i32", [P, I, I, P])
    bind("e2ekt_ola_norm_stream", [P, LL, LL, P, LL, P, P, P, I, LL, LL, LL, I, I, I, P])
    _lib = lib
    return lib


def version() -> str:
    return load().e2ekt_denoiser_version().decode()


def stft_pad(wav, wav_bs, n_valid, out, B, R, filter_length, hop, stream=None):
    return _msg(load().e2ekt_stft_pad(wav, wav_bs, n_valid, out, B, R, filter_length, hop, stream))


def spectral_subtract(spec, bias, frames, B, R, Cpad, filter_length, n_overlap, strength, stream=None):
    return _msg(load().e2ekt_spectral_subtract(spec, bias, frames, B, R, Cpad, filter_length, n_overlap, strength, stream))


def bias_frame(spec_row, bias, filter_length, stream=None):
    return _msg(load().e2ekt_bias_frame(spec_row, bias, filter_length, stream))


def ola_norm(y, in_, in_bs, n_valid, frames, win_sq, wav, pcm, B, n, R, filter_length, hop, stream=None):
    return _msg(load().e2ekt_ola_norm(y, in_, in_bs, n_valid, frames, win_sq, wav, pcm, B, n, R, filter_length, hop, stream))


def stft_pad_stream(seg, seg_bs, out, B, L, Rq, filter_length, hop, left_real, right_real, stream=None):
    return _msg(load().e2ekt_stft_pad_stream(seg, seg_bs, out, B, L, Rq, filter_length, hop, int(left_real), int(right_real), stream))


def fill_i32(p, n, v, stream=None):
    return _msg(load().e2ekt_fill_i32(p, n, v, stream))


def ola_norm_stream(y, y_bs, y_off, in_, in_bs, win_sq, wav, pcm, B, n, p_abs0, F_abs, filter_length, hop, pass_, stream=None):
    return _msg(load().e2ekt_ola_norm_stream(y, y_bs, y_off, in_, in_bs, win_sq, wav, pcm, B, n, p_abs0, F_abs, filter_length, hop, int(pass_), stream))
