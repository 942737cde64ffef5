"""ctypes binding of include/e2etts_compare.h (libe2etts_compare.so): two recordings compared on the GPU -- dynamic time warping over
cepstra of their log-mel, and along the path the mel-cepstral distortion, the mel L1, the f0 error and the voiced/unvoiced error.

The definition in the header is the contract.  The distortion is computed on DCT cepstra of THIS PROJECT'S log-mel: it is not comparable
with the SPTK / WORLD mel-cepstrum MCD figures of the literature.  The reference's only evaluation tool (modules/metrics/mos_test.py)
loads a learned metric; nothing here restates it.

The library loads without a GPU and ``Comparator(...)`` opens no device before a side is set.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_compare.h)
from ._lib import _addr, _expect, _is_cuda

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_compare.so")
# the TEST build of the same source (-DE2ECMP_TEST_HOOKS: two more exports, the e2ecmp_debug_* entry points), loaded instead of the
# product library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_compare_test.so")
ABI_VERSION = 1   # E2ECMP_ABI_VERSION of the include/e2etts_compare.h this binding mirrors
MAX_B, MAX_T, MAX_D, MAX_MEL = 4096, 4096, 64, 1024
A, B = 0, 1          # E2ECMP_A, E2ECMP_B
DTW, SYNC = 0, 1     # E2ECMP_DTW, E2ECMP_SYNC
MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)


class CResult(C.Structure):   # e2ecmp_result
    _fields_ = [("n_path", C.c_int64), ("n_voiced_both", C.c_int64), ("n_vuv_mismatch", C.c_int64), ("status", C.c_int64),
                ("dist_total", C.c_double), ("mcd_db", C.c_double), ("mel_l1", C.c_double), ("f0_rmse_hz", C.c_double),
                ("f0_rmse_cents", C.c_double)]


RESULT_DTYPE = np.dtype([(n, "<i8") for n in ("n_path", "n_voiced_both", "n_vuv_mismatch", "status")]
                        + [(n, "<f8") for n in ("dist_total", "mcd_db", "mel_l1", "f0_rmse_hz", "f0_rmse_cents")])

_P, _I, _SZ, _LL = C.c_void_p, C.c_int, C.c_size_t, C.c_longlong
# every entry point include/e2etts_compare.h declares, and all the library exports (tests/test_compare_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2ecmp_version": (C.c_char_p, []),
    "e2ecmp_abi_version": (_I, []),
    "e2ecmp_last_error": (C.c_char_p, [_P]),
    "e2ecmp_create": (_I, [_I, _I, _I, C.POINTER(_P)]),
    "e2ecmp_destroy": (None, [_P]),
    "e2ecmp_load": (_I, [_P, _P]),
    "e2ecmp_stream": (_P, [_P]),
    "e2ecmp_order_after": (_I, [_P, _P]),
    "e2ecmp_sync": (_I, [_P]),
    "e2ecmp_device_bytes": (_SZ, [_P]),
    "e2ecmp_set_mels": (_I, [_P, _I, _P, _P, _P, _I, _I]),
    "e2ecmp_set_features": (_I, [_P, _I, _P, _P, _I, _I, _I]),
    "e2ecmp_fetch_features": (_I, [_P, _I, _P]),
    "e2ecmp_run": (_I, [_P, _I, _LL, _P]),
    "e2ecmp_fetch_path": (_I, [_P, _I, _P, _LL, C.POINTER(_LL)]),
    "e2ecmp_profile_enable": (_I, [_P, _I]),
    "e2ecmp_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {
    "e2ecmp_debug_poison_workspace": (_I, [_P]),
    "e2ecmp_debug_run": (_I, [_P, _I, _LL, _P]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree comparison library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2ecmp", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


def dct_matrix(n: int) -> np.ndarray:
    """The orthonormal DCT-II matrix [n, n] in float64: C[k, m] = s_k cos(pi (m + 0.5) k / n), s_0 = sqrt(1 / n), s_k = sqrt(2 / n); C @ x is
    ``scipy.fft.dct(x, type=2, norm="ortho")`` and C is ``scipy.fft.dct(np.eye(n), type=2, norm="ortho", axis=0)``."""
    n = int(n)
    k, m = np.arange(n, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
    c = np.sqrt(2.0 / n) * np.cos(np.pi * (m + 0.5) * k / n)
    c[0] = np.sqrt(1.0 / n)
    return c


def default_basis(n_mel: int = 80, n_cep: int = 13) -> np.ndarray:
    """[n_cep, n_mel] float32: rows 1 .. n_cep of the orthonormal DCT-II, built in float64 and rounded once -- the cepstra of a frame are
    its DCT without c0, the frame's mean level."""
    if not 1 <= int(n_cep) <= int(n_mel) - 1:
        raise ValueError(f"the default basis has n_cep in [1, n_mel - 1] (got n_cep {n_cep}, n_mel {n_mel})")
    return dct_matrix(n_mel)[1:int(n_cep) + 1].astype(np.float32)


def _shape(x):
    return tuple(int(s) for s in x.shape)


def _f32(x, name):
    """numpy -> C-contiguous float32; torch tensors and resident tensors must be float32 and contiguous already."""
    if x is None:
        return None
    if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
        return np.ascontiguousarray(x, dtype=np.float32)
    if str(x.dtype).replace("torch.", "") != "float32":
        raise TypeError(f"{name}: dtype {x.dtype}, expected float32")
    return x if x.is_contiguous() else x.contiguous()


def _lens(lens, B: int) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens), dtype=np.int64).reshape(-1)
    if a.shape != (B,):
        raise ValueError(f"lens: {a.size} elements, expected {B}")
    return a


class Comparator(_companion.CompanionHandle):
    """One e2ecmp_handle: two resident sides and their comparison.  ``basis`` [n_cep, n_mel] float32 (default: ``default_basis``).
    Inputs are numpy arrays or torch tensors (host or GPU), or what lies resident in a ``mel.MelFrontend`` / ``f0.PitchTracker``."""
    _prefix, _what, _phases = "e2ecmp", "compare", ("cepstra", "search", "walk")

    def __init__(self, n_mel: int = 80, n_cep: int = 13, basis=None, device: Optional[int] = None):
        self.lib = load_library()
        self.n_mel, self.n_cep, self.device = int(n_mel), int(n_cep), int(device or 0)
        self.basis = default_basis(self.n_mel, self.n_cep) if basis is None else np.ascontiguousarray(basis, dtype=np.float32)
        if self.basis.shape != (self.n_cep, self.n_mel):
            raise ValueError(f"basis of shape {self.basis.shape}, expected {(self.n_cep, self.n_mel)}")
        h = C.c_void_p()
        rc = self.lib.e2ecmp_create(self.device, self.n_mel, self.n_cep, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2ecmp_last_error(None).decode())
        self._h = h
        self._loaded = False
        self._sides = [None, None]   # (B, T, D) of a set side
        self._pairs = None           # (lens_a, lens_b) of the last run

    def _load(self):
        if not self._loaded:
            self._check(self.lib.e2ecmp_load(self._h, self.basis.ctypes.data), "e2ecmp_load")
            self._loaded = True

    @staticmethod
    def _side(side) -> int:
        if side in ("a", "A", A):
            return A
        if side in ("b", "B", B):
            return B
        raise ValueError(f"side must be 'a' or 'b' (got {side!r})")

    def order_after_stream(self, stream: int):
        """Order this handle's stream after everything queued on ``stream`` (a raw hipStream_t, e.g. another library's)."""
        self._call("order_after", stream)

    def hip_stream(self) -> int:
        return _companion.CompanionHandle.stream(self)

    def set_mels(self, side, mel, lens, f0=None):
        """One side from log-mel [B, T, n_mel] float32 and, optionally, its f0 track [B, T] in Hz (0 = unvoiced); lens [B] frames.  ``mel``
        may be a ``MelFrontend`` and ``f0`` a ``PitchTracker``: what their last forward left resident is read where it lies, this
        handle's stream ordered after theirs.  The side is copied and stays resident until it is set again."""
        side = self._side(side)
        if hasattr(mel, "resident") and hasattr(mel, "n_fft"):        # a MelFrontend
            self.order_after_stream(mel.stream())
            mel = mel.resident()[0]
        if f0 is not None and hasattr(f0, "resident") and hasattr(f0, "hip_stream"):   # a PitchTracker
            self.order_after_stream(f0.hip_stream())
            f0 = f0.resident()
        mel = _f32(mel, "mel")
        f0 = _f32(f0, "f0")
        shp = _shape(mel)
        if len(shp) != 3 or shp[2] != self.n_mel:
            raise ValueError(f"expected mel of shape [B, T, {self.n_mel}], got {shp}")
        Bn, T = shp[0], shp[1]
        if f0 is not None and _shape(f0) != (Bn, T):
            raise ValueError(f"f0 of shape {_shape(f0)}, expected {(Bn, T)}")
        ln = _lens(lens, Bn)
        _expect(mel, "mel", "float32", Bn * T * self.n_mel)
        _expect(f0, "f0", "float32", Bn * T)
        self._load()
        self._order(mel, f0)
        self._sides[side] = None
        self._call("set_mels", side, _addr(mel), _addr(f0), ln.ctypes.data, Bn, T)
        self._sides[side] = (Bn, T, self.n_cep)

    def set_a(self, mel, lens, f0=None):
        self.set_mels(A, mel, lens, f0)

    def set_b(self, mel, lens, f0=None):
        self.set_mels(B, mel, lens, f0)

    def set_features(self, side, features, lens):
        """One side from ready features [B, T, D] float32, D <= 64: a general DTW (no mel L1, no f0 figures)."""
        side = self._side(side)
        x = _f32(features, "features")
        shp = _shape(x)
        if len(shp) != 3:
            raise ValueError(f"expected features of shape [B, T, D], got {shp}")
        ln = _lens(lens, shp[0])
        _expect(x, "features", "float32", shp[0] * shp[1] * shp[2])
        self._order(x)
        self._sides[side] = None
        self._call("set_features", side, _addr(x), ln.ctypes.data, shp[0], shp[1], shp[2])
        self._sides[side] = shp

    def features(self, side, out=None) -> np.ndarray:
        """The features the search reads of a side, [B, T, D] float32: the cepstra of a side set from mels (rows past a length are 0)."""
        side = self._side(side)
        if self._sides[side] is None:
            raise RuntimeError("the side is not set")
        if out is None:
            out = np.empty(self._sides[side], np.float32)
        _expect(out, "out", "float32", int(np.prod(self._sides[side])))
        self._order(out)
        self._call("fetch_features", side, _addr(out))
        return out

    def run(self, mode: str = "dtw", band: Optional[int] = None, return_path: bool = False, _entry: str = "run"):
        """Compares the sides pair by pair -> a list of dicts, one per pair, with the fields of e2ecmp_result (``n_path``, ``dist_total``,
        ``mcd_db``, ``mel_l1``, ``f0_rmse_hz``, ``f0_rmse_cents``, ``n_voiced_both``, ``n_vuv_mismatch``, ``status``) and, with
        ``return_path``, ``path`` [n_path, 2] int32 in path order.  ``mode``: "dtw", or "sync" for the frame-synchronous path (i, i).
        ``band``: None for none, or the Sakoe-Chiba band's half width in frames of the shorter sequence, at least 1."""
        if mode not in ("dtw", "sync"):
            raise ValueError(f"mode must be 'dtw' or 'sync' (got {mode!r})")
        if self._sides[A] is None or self._sides[B] is None:
            raise RuntimeError("run before both sides are set")
        n = self._sides[A][0]
        res = np.zeros(n, RESULT_DTYPE)
        self._call(_entry, DTW if mode == "dtw" else SYNC, -1 if band is None else int(band), res.ctypes.data)
        out = []
        for b in range(n):
            d = {k: (int(res[k][b]) if res.dtype[k].kind == "i" else float(res[k][b])) for k in res.dtype.names}
            if return_path:
                p = np.empty((d["n_path"], 2), np.int32)
                got = C.c_longlong(0)
                self._call("fetch_path", b, p.ctypes.data if p.size else None, d["n_path"], C.byref(got))
                assert got.value == d["n_path"]
                d["path"] = p
            out.append(d)
        return out

    def poison_workspace(self):
        super().poison_workspace()
        self._sides = [None, None]

    def debug_run(self, mode: str = "dtw", band: Optional[int] = None, return_path: bool = False):
        """Test build only (E2ETTS_TEST_HOOKS=1): ``run`` that also takes band = 0, the cells exactly on the line i * Tb == j * Ta."""
        if not hasattr(self.lib, "e2ecmp_debug_run"):
            raise RuntimeError("debug_run needs the test build of the compare library (E2ETTS_TEST_HOOKS=1)")
        return self.run(mode, band, return_path, _entry="debug_run")


def compare_audio(wav_a, lens_a, wav_b, lens_b, sample_rate: int, hop: int, n_fft: int = 1024, win_length: Optional[int] = None, n_mel: int = 80,
                  fmin: float = 0.0, fmax: Optional[float] = 8000.0, n_cep: int = 13, mode: str = "dtw", band: Optional[int] = None,
                  return_path: bool = False, with_f0: bool = True, device: Optional[int] = None, mel_basis=None, clip_val: float = 1e-5):
    """Two batches of recordings compared: wav_a, wav_b [B, n] (float32 in [-1, 1] or int16 PCM; numpy or torch, host or GPU) with lens_a,
    lens_b [B] samples -> ``Comparator.run``'s list of dicts.  Per side the mel front-end (e2e_tts_amd.mel, the reference's transform) and,
    with ``with_f0``, the pitch tracker (e2e_tts_amd.f0) read the samples; the comparator reads their results where they lie in HBM, its
    stream ordered after theirs: nothing passes through the host between them.  Utterances shorter than one hop are refused."""
    from .f0 import PitchTracker
    from .mel import MelFrontend, dft_basis, mel_filterbank
    dev = int(device or 0)
    fe = MelFrontend(n_fft, hop, n_mel, device=dev)
    fe.load(dft_basis(n_fft, win_length), mel_filterbank(sample_rate, n_fft, n_mel, fmin, fmax) if mel_basis is None else mel_basis, clip_val)
    trk = PitchTracker(sample_rate, hop, device=dev) if with_f0 else None
    cmp_ = Comparator(n_mel, n_cep, device=dev)
    try:
        for side, wav, ln in ((A, wav_a, lens_a), (B, wav_b, lens_b)):
            r = fe.forward(wav, ln, want=())
            if trk is not None:
                t = trk.forward(wav, ln, want=())
                if t["T"] != r["T"] or not np.array_equal(t["lens"], r["mel_lens"]):
                    raise RuntimeError("the pitch track and the mel are on different grids")
            cmp_.set_mels(side, fe, r["mel_lens"], trk)
        return cmp_.run(mode, band, return_path)
    finally:
        cmp_.close()
        fe.close()
        if trk is not None:
            trk.close()
