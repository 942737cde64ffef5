"""ctypes binding of include/e2etts_f0.h (libe2etts_f0.so): the f0 track of a recording on the mel front-end's frame grid, and the data
loader's pitch targets (get_f0) made from it, on the GPU.

The reference gets its track from parselmouth (src/tools/utils.py: extract_f0).  The library is Boersma's autocorrelation method as
Praat documents it, restated, and is UNPINNED AGAINST PARSELMOUTH (parselmouth is not a dependency and was never run beside it): the
definition in the header is the contract.  Frames lie on the mel grid, so a track has exactly mel_len frames; the reference's truncation
and zero padding onto the mel length is not reproduced.

The library loads without a GPU and ``PitchTracker(...)`` opens no device before its tables are loaded.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Mapping, Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_f0.h)
from ._lib import _addr, _expect
from .mel import ResidentTensor
from .resample import _audio_layout

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_f0.so")
# the TEST build of the same source (-DE2EF0_TEST_HOOKS: four more exports, the e2ef0_debug_* entry points), loaded instead of the product
# library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_f0_test.so")
ABI_VERSION = 1   # E2EF0_ABI_VERSION of the include/e2etts_f0.h this binding mirrors
MAX_B, MAX_K, MIN_RATE, MAX_RATE = 4096, 16, 1000, 384000
F32, I16 = 0, 1        # E2EF0_F32, E2EF0_I16
LINEAR, LOG = 0, 1     # E2EF0_LINEAR, E2EF0_LOG
# what the reference passes to to_pitch_ac (floor, ceiling, voicing_threshold), then Praat's defaults
DEFAULTS = dict(floor=80.0, ceiling=750.0, voicing_threshold=0.5, silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35,
                voiced_unvoiced_cost=0.14, max_candidates=15)


class CParams(C.Structure):   # e2ef0_params
    _fields_ = [("struct_size", C.c_size_t), ("floor", C.c_double), ("ceiling", C.c_double), ("voicing_threshold", C.c_double),
                ("silence_threshold", C.c_double), ("octave_cost", C.c_double), ("octave_jump_cost", C.c_double), ("voiced_unvoiced_cost", C.c_double),
                ("max_candidates", C.c_int)]


_P, _I, _D, _SZ, _LL = C.c_void_p, C.c_int, C.c_double, C.c_size_t, C.c_longlong
# every entry point include/e2etts_f0.h declares, and all the library exports (tests/test_f0_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2ef0_version": (C.c_char_p, []),
    "e2ef0_abi_version": (_I, []),
    "e2ef0_last_error": (C.c_char_p, [_P]),
    "e2ef0_create": (_I, [_I, _I, _I, C.POINTER(_P)]),
    "e2ef0_destroy": (None, [_P]),
    "e2ef0_configure": (_I, [_P, C.POINTER(CParams), _P, _P]),
    "e2ef0_window": (_I, [_I, _I, _D, _D]),
    "e2ef0_lags": (_I, [_I, _I, _D, _D]),
    "e2ef0_tau_min": (_I, [_I, _I, _D, _D]),
    "e2ef0_tile_frames": (_I, [_P]),
    "e2ef0_stream": (_P, [_P]),
    "e2ef0_order_after": (_I, [_P, _P]),
    "e2ef0_sync": (_I, [_P]),
    "e2ef0_device_bytes": (_SZ, [_P]),
    "e2ef0_forward": (_I, [_P, _P, _I, _LL, _P, _I, _LL, _P, _P, C.POINTER(_I)]),
    "e2ef0_targets": (_I, [_P, _D, _D, _I, _D, _P, _P]),
    "e2ef0_f0_dev": (_P, [_P]),
    "e2ef0_target_f0_dev": (_P, [_P]),
    "e2ef0_target_uv_dev": (_P, [_P]),
    "e2ef0_profile_enable": (_I, [_P, _I]),
    "e2ef0_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {
    "e2ef0_debug_poison_workspace": (_I, [_P]),
    "e2ef0_debug_acf": (_I, [_P, _P, _I, _LL, _P, _I, _LL, _P, C.POINTER(_I)]),
    "e2ef0_debug_candidates": (_I, [_P, _P, _I, _LL, _P, _I, _LL, _P, _P, C.POINTER(_I)]),
    "e2ef0_debug_path": (_I, [_P, _P, _P, _P, _I, _I, _P]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree pitch library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2ef0", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


# ---- the host half of the definition
def geometry(sr: int, floor: float = 80.0, ceiling: float = 750.0):
    """(W, tau_min, tau_max) of the header's definition: W = floor(3 sr / floor), plus 1 if that is even; tau_max = floor(sr / floor);
    tau_min = ceil(sr / ceiling)."""
    W = int(math.floor(3.0 * sr / floor))
    W += 1 - W % 2
    return W, int(math.ceil(sr / ceiling)), int(math.floor(sr / floor))


def window_tables(sr: int, floor: float = 80.0):
    """(w [W], r_w [tau_max + 2]) float32: the Hann window w[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / W) and its own normalised autocorrelation
    r_w[tau] = sum_i w[i] w[i + tau] / sum_i w[i]^2, built in float64 and rounded once."""
    W, _, tau_max = geometry(sr, floor)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W, dtype=np.float64) + 0.5) / W)
    full = np.correlate(w, w, mode="full")[W - 1:]
    return w.astype(np.float32), (full[:tau_max + 2] / full[0]).astype(np.float32)


def frames_of(n_valid, hop: int) -> np.ndarray:
    """Frames of rows with n_valid samples: floor(n_valid / hop), the mel front-end's mel_lens."""
    return np.asarray(n_valid, np.int64) // int(hop)


def _n_valid(n_valid, B: int, n: int):
    if n_valid is None:
        return np.full(B, n, np.int64)
    nv = np.ascontiguousarray(np.asarray(n_valid.cpu() if hasattr(n_valid, "cpu") else n_valid), dtype=np.int64).reshape(-1)
    if nv.shape != (B,):
        raise ValueError(f"n_valid: {nv.size} elements, expected {B}")
    return nv


class PitchTracker(_companion.CompanionHandle):
    """One e2ef0_handle for recordings at ``sample_rate`` Hz on the mel grid of ``hop``.  ``params``: the fields of e2ef0_params (``DEFAULTS``).
    Inputs are numpy arrays or torch tensors (float32 in [-1, 1] or int16 PCM), on the host or the GPU."""
    _prefix, _what, _phases = "e2ef0", "f0", ("analyse", "path", "targets")

    def __init__(self, sample_rate: int, hop: int, device: Optional[int] = 0, **params):
        unknown = sorted(set(params) - set(DEFAULTS))
        if unknown:
            raise ValueError(f"unknown parameters {unknown} (known: {sorted(DEFAULTS)})")
        self.lib = load_library()
        self.sample_rate, self.hop, self.device = int(sample_rate), int(hop), int(device or 0)
        self.params = {**DEFAULTS, **params}
        self.K = int(self.params["max_candidates"])
        h = C.c_void_p()
        rc = self.lib.e2ef0_create(self.device, self.sample_rate, self.hop, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2ef0_last_error(None).decode())
        self._h = h
        self._resident = None
        self._configured = False
        fl, ce = float(self.params["floor"]), float(self.params["ceiling"])
        self.W = self.lib.e2ef0_window(self.sample_rate, self.hop, fl, ce)
        self.lags = self.lib.e2ef0_lags(self.sample_rate, self.hop, fl, ce)
        self.tau_min = self.lib.e2ef0_tau_min(self.sample_rate, self.hop, fl, ce)
        if self.W < 0 or not 2 <= self.K <= MAX_K:
            self._configure()   # raises with the library's message, before a device is opened

    def _configure(self):
        """Loads the parameters and the window tables (opens the device): before the first computing call."""
        if self._configured:
            return
        p = CParams(C.sizeof(CParams), *(float(self.params[k]) for k in list(DEFAULTS)[:-1]), self.K)
        if self.W < 0:   # a refused geometry: tables of a size the library never reads (it checks the geometry first)
            w, rw = np.zeros(1, np.float32), np.ones(1, np.float32)
        else:
            w, rw = window_tables(self.sample_rate, float(self.params["floor"]))
            assert w.size == self.W and rw.size == self.lags
        try:
            self._check(self.lib.e2ef0_configure(self._h, C.byref(p), w.ctypes.data, rw.ctypes.data), "e2ef0_configure")
        except ValueError:
            self.close()
            raise
        self._configured = True

    @property
    def tile_frames(self) -> int:
        self._configure()
        return int(self.lib.e2ef0_tile_frames(self._h))

    def _audio(self, wavs, n_valid):
        x, dt, _, B, n, stride, addr = _audio_layout(wavs, "wavs")
        nv = _n_valid(n_valid, B, n)
        if n < 1 or (nv < 0).any() or (nv > n).any():
            raise ValueError(f"n_valid must lie in [0, n = {n}] and n must be at least 1")
        T = int(frames_of(nv, self.hop).max())
        if T < 1:
            raise ValueError(f"no row holds a frame: need n_valid >= hop = {self.hop} in at least one row")
        return x, dt, B, n, stride, addr, nv, T

    def forward(self, wavs, n_valid=None, want=("f0",), out_f0=None):
        """wavs [B, n], n_valid [B] or None -> dict with "T", "lens" [B] int64 (the mel front-end's mel_lens) and, when ``want`` names it,
        "f0" [B, T] float32 Hz (0 = unvoiced; 0 in frames >= lens).  ``out_f0``: an array or tensor (host or GPU) to write instead.  The
        track stays resident (``resident()``, ``targets()``) until the next forward."""
        x, dt, B, n, stride, addr, nv, T = self._audio(wavs, n_valid)
        self._configure()
        r = {}
        if out_f0 is None and "f0" in want:
            out_f0 = r["f0"] = np.empty((B, T), np.float32)
        _expect(out_f0, "out_f0", "float32", B * T)
        lens = np.zeros(B, np.int64)
        t_out = C.c_int(0)
        self._order(x, out_f0)
        self._check(self.lib.e2ef0_forward(self._h, addr, dt, stride, nv.ctypes.data, B, n, _addr(out_f0), lens.ctypes.data, C.byref(t_out)), "e2ef0_forward")
        assert t_out.value == T
        r["T"], r["lens"] = T, lens
        self._resident = (B, T)
        return r

    def targets(self, stats: Optional[Mapping[str, object]] = None, pitch_quantization: str = "linear", pitch_eps: float = 1e-9, out_f0=None, out_uv=None,
                fetch: bool = True):
        """The data loader's get_f0 on the resident track -> (f0 target, uv target) [B, T] float32 numpy arrays (None with ``fetch=False``
        or when ``out_f0`` / ``out_uv``, arrays or tensors on the host or the GPU, are given).  ``stats``: {"f0": {"mean", "std"}} for
        "linear"; "log" takes log2(f0 + pitch_eps).  Both stay resident (``resident_targets()``)."""
        if pitch_quantization not in ("linear", "log"):
            raise ValueError(f"pitch_quantization must be 'linear' or 'log' (got {pitch_quantization!r})")
        if self._resident is None:
            raise RuntimeError("targets without a resident track (no forward has completed)")
        B, T = self._resident
        mean = std = 0.0
        if pitch_quantization == "linear":
            if stats is None:
                raise ValueError("linear targets need stats['f0']['mean'] and ['std']")
            mean, std = float(stats["f0"]["mean"]), float(stats["f0"]["std"])
        given = out_f0 is not None or out_uv is not None
        if fetch and not given:
            out_f0, out_uv = np.empty((B, T), np.float32), np.empty((B, T), np.float32)
        _expect(out_f0, "out_f0", "float32", B * T)
        _expect(out_uv, "out_uv", "float32", B * T)
        self._order(out_f0, out_uv)
        self._call("targets", mean, std, LINEAR if pitch_quantization == "linear" else LOG, float(pitch_eps), _addr(out_f0), _addr(out_uv))
        return (out_f0, out_uv) if fetch and not given else None

    def resident(self):
        """The track [B, T] of the last forward as a ResidentTensor view of the handle's HBM."""
        p = self.lib.e2ef0_f0_dev(self._h)
        if not p:
            raise RuntimeError("nothing is resident (no forward has completed)")
        return ResidentTensor(p, self._resident)

    def resident_targets(self):
        """(f0 target, uv target) [B, T] of the last ``targets`` as ResidentTensor views."""
        fp, up = self.lib.e2ef0_target_f0_dev(self._h), self.lib.e2ef0_target_uv_dev(self._h)
        if not fp or not up:
            raise RuntimeError("no targets are resident")
        return ResidentTensor(fp, self._resident), ResidentTensor(up, self._resident)

    def hip_stream(self) -> int:
        return _companion.CompanionHandle.stream(self)

    def order_after_stream(self, stream: int):
        """Order this handle's stream after everything queued on ``stream`` (a raw hipStream_t, e.g. another library's)."""
        self._call("order_after", stream)

    def poison_workspace(self):
        super().poison_workspace()
        self._resident = None

    # ---- test build only (E2ETTS_TEST_HOOKS=1)
    def debug_acf(self, wavs, n_valid=None):
        """The analysis kernel with r written out -> r [B, T, tau_max + 2] float32."""
        x, dt, B, n, stride, addr, nv, T = self._audio(wavs, n_valid)
        self._configure()
        r = np.empty((B, T, self.lags), np.float32)
        t_out = C.c_int(0)
        self._order(x)
        self._hook("acf", addr, dt, stride, nv.ctypes.data, B, n, r.ctypes.data, C.byref(t_out))
        self._resident = None
        return r

    def debug_candidates(self, wavs, n_valid=None):
        """-> (freq, strength) [B, T, K] float32 as the path search reads them."""
        x, dt, B, n, stride, addr, nv, T = self._audio(wavs, n_valid)
        self._configure()
        f, s = np.empty((B, T, self.K), np.float32), np.empty((B, T, self.K), np.float32)
        t_out = C.c_int(0)
        self._order(x)
        self._hook("candidates", addr, dt, stride, nv.ctypes.data, B, n, f.ctypes.data, s.ctypes.data, C.byref(t_out))
        self._resident = None
        return f, s

    def debug_path(self, freq, strength, frames):
        """The path kernel alone on the caller's candidates [B, T, K] (float32 numpy; an empty slot has strength -inf) -> f0 [B, T], which
        stays resident with ``frames`` as the rows' lengths."""
        f = np.ascontiguousarray(freq, dtype=np.float32)
        s = np.ascontiguousarray(strength, dtype=np.float32)
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        if f.ndim != 3 or f.shape != s.shape or f.shape[2] != self.K or fr.shape != (f.shape[0],):
            raise ValueError(f"freq {f.shape}, strength {s.shape}, frames {fr.shape}: expected [B, T, {self.K}] twice and [B]")
        self._configure()
        out = np.empty(f.shape[:2], np.float32)
        self._hook("path", f.ctypes.data, s.ctypes.data, fr.ctypes.data, f.shape[0], f.shape[1], out.ctypes.data)
        self._resident = out.shape   # resident as a forward's track: ``targets`` can be run on it
        return out
