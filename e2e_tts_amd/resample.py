"""ctypes binding of include/e2etts_resample.h (libe2etts_resample.so): sample-rate conversion by a rational ratio L / M on the GPU -- a
polyphase FIR, batched and streaming -- and the default filter it is loaded with.

The reference converts rates through pydub.set_frame_rate (modules/metrics/audio_processing.py:26), i.e. audioop.ratecv: linear
interpolation without an anti-aliasing filter.  That is not reproduced.  The arithmetic here is the header's: with taps ``h`` the result
equals ``scipy.signal.resample_poly(x, L, M, window=h / L)``.

The library loads without a GPU and ``Resampler(...)`` opens no device before its filter is loaded at the first use.  There is no CPU
fallback."""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
from typing import Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_resample.h)
from ._lib import _addr, _expect, _is_cuda

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_resample.so")
# the TEST build of the same source (-DE2ERS_TEST_HOOKS: one more export, e2ers_debug_poison_workspace), loaded instead of the product
# library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_resample_test.so")
ABI_VERSION = 1   # E2ERS_ABI_VERSION of the include/e2etts_resample.h this binding mirrors
F32, I16 = 0, 1   # E2ERS_F32, E2ERS_I16
MAX_B, MAX_RATIO, MAX_PHASE_TAPS = 4096, 1024, 1024

_P, _I, _SZ, _LL = C.c_void_p, C.c_int, C.c_size_t, C.c_longlong
# every entry point include/e2etts_resample.h declares, and all the library exports (tests/test_resample_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2ers_version": (C.c_char_p, []),
    "e2ers_abi_version": (_I, []),
    "e2ers_last_error": (C.c_char_p, [_P]),
    "e2ers_create": (_I, [_I, C.POINTER(_P)]),
    "e2ers_destroy": (None, [_P]),
    "e2ers_load": (_I, [_P, _P, _I, _I, _I]),
    "e2ers_stream": (_P, [_P]),
    "e2ers_order_after": (_I, [_P, _P]),
    "e2ers_sync": (_I, [_P]),
    "e2ers_device_bytes": (_SZ, [_P]),
    "e2ers_forward": (_I, [_P, _P, _I, _LL, _P, _I, _LL, _P, _P, _LL, _P, C.POINTER(_LL)]),
    "e2ers_wav_dev": (_P, [_P]),
    "e2ers_pcm_dev": (_P, [_P]),
    "e2ers_stream_begin": (_I, [_P, _I, _I]),
    "e2ers_stream_push": (_I, [_P, _P, _LL, _LL, _I, C.POINTER(_LL)]),
    "e2ers_stream_fetch": (_I, [_P, _P, _P, _LL, _SZ]),
    "e2ers_tile_outputs": (_LL, [_P]),
    "e2ers_profile_enable": (_I, [_P, _I]),
    "e2ers_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {"e2ers_debug_poison_workspace": (_I, [_P])}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree resample library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2ers", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


def ratio(src_rate: int, dst_rate: int):
    """(L, M) in lowest terms: dst_rate / src_rate = L / M."""
    src_rate, dst_rate = int(src_rate), int(dst_rate)
    if src_rate < 1 or dst_rate < 1:
        raise ValueError(f"rates must be positive (got {src_rate} -> {dst_rate})")
    g = math.gcd(src_rate, dst_rate)
    return dst_rate // g, src_rate // g


def n_out(n, L: int, M: int):
    """ceil(n * L / M), the outputs of n input samples (numbers or integer arrays)."""
    return -((-np.asarray(n, np.int64) * int(L)) // int(M))


def design(src_rate: int, dst_rate: int, zeros: int = 16, beta: float = 8.6, rolloff: float = 0.9):
    """The default filter -> (taps float32 [2 * half + 1], L, M): a Kaiser-windowed sinc built in float64 and rounded once.
    q = max(L, M), half = zeros * q, fc = rolloff / q; h[j] = fc * sinc(fc * (j - half)) * kaiser(2 * half + 1, beta)[j], scaled so that
    sum(h) = L (unity gain after the zero-stuffing by L)."""
    L, M = ratio(src_rate, dst_rate)
    q = max(L, M)
    half = int(zeros) * q
    if half < 1:
        raise ValueError("zeros must be at least 1")
    fc = float(rolloff) / q
    j = np.arange(2 * half + 1, dtype=np.float64) - half
    h = fc * np.sinc(fc * j) * np.kaiser(2 * half + 1, float(beta))
    h *= L / h.sum()
    return h.astype(np.float32), L, M


def response(taps, L: int, M: int, n_fft: int = 1 << 22):
    """Host-side figures of a filter, from an n_fft-point FFT of the taps (frequencies relative to the rate L x the input rate, at which the
    taps run; "lower Nyquist" = 0.5 / max(L, M) there) -> dict:
    ``ripple_db``     max |20 log10(|H| / L)| up to 0.7 x the lower Nyquist,
    ``stopband_db``   max 20 log10(|H| / L) from 1.1 x the lower Nyquist,
    ``phase_dc_err``  max over the L phases r of |sum_i h[r + i L] - 1|: the gain each output phase applies to a constant."""
    h = np.asarray(taps, np.float64).reshape(-1)
    L, M = int(L), int(M)
    n_fft = max(int(n_fft), 1 << int(np.ceil(np.log2(h.size * 8))))
    H = np.abs(np.fft.rfft(h, n_fft)) / L
    f = np.arange(H.size) / n_fft
    nyq = 0.5 / max(L, M)
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(H)
    phase = np.array([h[r::L].sum() for r in range(L)])
    return {"ripple_db": float(np.abs(db[f <= 0.7 * nyq]).max()), "stopband_db": float(db[f >= 1.1 * nyq].max()),
            "phase_dc_err": float(np.abs(phase - 1.0).max())}


class ResidentAudio:
    """A [B, n] tensor in a handle's HBM, given by its raw device address (what ``_addr`` / ``_expect`` / ``_is_cuda`` need to hand it to
    another library's entry point).  Valid until the owning handle's next forward."""
    is_cuda = True

    def __init__(self, ptr: int, shape, dtype: str):
        self.ptr, self.shape, self.dtype, self.ndim = int(ptr), tuple(int(s) for s in shape), dtype, len(shape)

    def data_ptr(self) -> int:
        return self.ptr

    def is_contiguous(self) -> bool:
        return True

    def numel(self) -> int:
        return int(np.prod(self.shape))

    def stride(self, d: int) -> int:
        return int(np.prod(self.shape[d + 1:]))


def _audio_layout(audio, what="audio"):
    """(audio or a contiguous copy, dtype code, element size, B, n, row stride in elements, address)"""
    if audio.ndim != 2:
        raise ValueError(f"expected {what} of shape [B, n], got {tuple(audio.shape)}")
    B, n = int(audio.shape[0]), int(audio.shape[1])
    is_np = isinstance(audio, np.ndarray)
    dt = audio.dtype.name if is_np else str(audio.dtype).replace("torch.", "")
    if dt not in ("float32", "int16"):
        raise TypeError(f"{what}: dtype {dt}, expected float32 or int16")
    esz = 4 if dt == "float32" else 2
    if is_np:
        if n and (audio.strides[1] != esz or (B > 1 and (audio.strides[0] % esz or audio.strides[0] < n * esz))):
            audio = np.ascontiguousarray(audio)
        stride, addr = (audio.strides[0] // esz if B > 1 and n else n), audio.ctypes.data
    else:
        if n and (audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n)):
            audio = audio.contiguous()
        stride, addr = (audio.stride(0) if B > 1 and n else n), audio.data_ptr()
    return audio, (F32 if dt == "float32" else I16), esz, B, n, int(stride), addr


class Resampler(_companion.CompanionHandle):
    """One e2ers_handle converting ``src_rate`` to ``dst_rate`` (``taps``: a filter of the caller's own for that ratio, odd in number;
    None: ``design``).  Inputs are numpy arrays or torch tensors, on the host or the GPU."""
    _prefix, _what, _phases = "e2ers", "resample", ("upload", "filter", "fetch")

    def __init__(self, src_rate: int, dst_rate: int, device: Optional[int] = None, taps=None, **design_args):
        self.lib = load_library()
        self.src_rate, self.dst_rate, self.device = int(src_rate), int(dst_rate), int(device or 0)
        self.L, self.M = ratio(src_rate, dst_rate)
        if taps is None:
            taps = design(src_rate, dst_rate, **design_args)[0]
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        h = C.c_void_p()
        rc = self.lib.e2ers_create(self.device, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2ers_last_error(None).decode())
        self._h = h
        self._loaded = False
        self._resident = None
        self._inflight = collections.deque(maxlen=4)

    def load(self):
        """Hands the filter to the library (the first touch of the GPU); ``forward`` and ``stream`` do it when needed."""
        if not self._loaded:
            self._check(self.lib.e2ers_load(self._h, self.taps.ctypes.data, int(self.taps.size), self.L, self.M), "e2ers_load")
            self._loaded = True
        return self

    @property
    def tile_outputs(self) -> int:
        self.load()
        return int(self.lib.e2ers_tile_outputs(self._h))

    def n_out(self, n):
        return n_out(n, self.L, self.M)

    def forward(self, x, n_valid=None, want=("wav",), out_wav=None, out_pcm=None, out_stride: Optional[int] = None):
        """x [B, n] float32 or int16 PCM (rows may be strided), n_valid [B] or None -> dict with "n_out" [B] int64 (numpy), "width" =
        ceil(n * L / M) and the numpy arrays named in ``want``: "wav" [B, width] float32, "pcm" [B, width] int16; samples at or past a
        row's n_out are 0.  ``out_wav`` / ``out_pcm``: arrays or tensors (host or GPU) to write instead, rows ``out_stride`` elements apart
        (default: width).  ``want=()`` without outputs computes only: the results stay resident (``resident()``)."""
        self.load()
        x, dt, _, B, n, stride, addr = _audio_layout(x)
        nv = None
        if n_valid is not None:
            nv = np.ascontiguousarray(np.asarray(n_valid.cpu() if hasattr(n_valid, "cpu") else n_valid), dtype=np.int64).reshape(-1)
            if nv.shape != (B,):
                raise ValueError(f"n_valid: {nv.size} elements, expected {B}")
        W = int(n_out(n, self.L, self.M))
        os_ = W if out_stride is None else int(out_stride)
        r = {}
        if n >= 1 and os_ >= W:   # (anything else the library refuses: nothing may be written)
            if out_wav is None and "wav" in want:
                out_wav = r["wav"] = np.empty((B, W), np.float32)
            if out_pcm is None and "pcm" in want:
                out_pcm = r["pcm"] = np.empty((B, W), np.int16)
            _expect(out_wav, "out_wav", "float32", (B - 1) * os_ + W, at_least=True)
            _expect(out_pcm, "out_pcm", "int16", (B - 1) * os_ + W, at_least=True)
        else:
            out_wav = out_pcm = None
        lens = np.zeros(B, np.int64)
        w_out = C.c_longlong(0)
        self._order(x, out_wav, out_pcm)
        self._check(self.lib.e2ers_forward(self._h, addr, dt, stride, None if nv is None else nv.ctypes.data, B, n, _addr(out_wav), _addr(out_pcm),
                                           os_, lens.ctypes.data, C.byref(w_out)), "e2ers_forward")
        assert w_out.value == W
        r["n_out"], r["width"] = lens, W
        self._resident = (B, W)
        return r

    def resident(self):
        """(wav [B, width] float32, pcm [B, width] int16) of the last forward as ResidentAudio views of the handle's HBM."""
        wp, pp = self.lib.e2ers_wav_dev(self._h), self.lib.e2ers_pcm_dev(self._h)
        if not wp or not pp:
            raise RuntimeError("nothing is resident (no forward has completed)")
        return ResidentAudio(wp, self._resident, "float32"), ResidentAudio(pp, self._resident, "int16")

    def hip_stream(self) -> int:
        """The handle's raw hipStream_t (``stream`` itself is the chunk generator below)."""
        return _companion.CompanionHandle.stream(self)

    def order_after_stream(self, stream: int):
        """Order this handle's stream after everything queued on ``stream`` (a raw hipStream_t, e.g. another library's)."""
        self._call("order_after", stream)

    # ---- streaming
    def stream_begin(self, B: int, dtype: int = F32):
        self.load()
        self._call("stream_begin", int(B), int(dtype))

    def stream_push(self, chunk, last: bool = False) -> int:
        """Appends chunk [B, n] (None: nothing, for a flush with ``last``); returns the outputs per row this push made."""
        n_ready = C.c_longlong(0)
        if chunk is None:
            self._call("stream_push", None, 0, 0, 1 if last else 0, C.byref(n_ready))
        else:
            chunk, _, _, _, n, stride, addr = _audio_layout(chunk, "chunk")
            self._inflight.append(chunk)   # device memory must outlive the copy the push enqueued (at most two pushes are unfetched)
            self._order(chunk)
            self._call("stream_push", addr if n else None, stride, n, 1 if last else 0, C.byref(n_ready))
        return int(n_ready.value)

    def stream_fetch(self, B: int, n_ready: int, want_pcm: bool = False):
        """The [B, n_ready] outputs of the oldest unfetched push (float32, or int16 PCM)."""
        out = np.empty((B, n_ready), np.int16 if want_pcm else np.float32)
        self._call("stream_fetch", None if want_pcm else _addr(out), _addr(out) if want_pcm else None, n_ready, out.size)
        return out

    def stream(self, chunks, want_pcm: bool = False):
        """Generator: feed an iterable of chunks [B, n] (numpy / torch, float32 or int16, all of one dtype and B), yield the converted
        pieces [B, n_ready] as they become final.  Concatenated along axis 1 they equal ``forward`` of the concatenated input bit for bit.
        Chunk i + 1 is pushed before chunk i's outputs are fetched, as ``Engine.vocoder_stream`` does."""
        chunks = iter(chunks)
        cur = next(chunks, None)
        if cur is None:
            return
        B = int(cur.shape[0])
        self.stream_begin(B, _audio_layout(cur, "chunk")[1])
        pend = collections.deque()   # outputs made by the unfetched pushes
        while cur is not None:
            nxt = next(chunks, None)
            made = self.stream_push(cur, last=nxt is None)
            out = None
            if made > 0:
                pend.append(made)
            if len(pend) == 2:
                out = self.stream_fetch(B, pend.popleft(), want_pcm)
            if out is not None:
                yield out
            cur = nxt
        while pend:
            yield self.stream_fetch(B, pend.popleft(), want_pcm)
