"""ctypes binding of include/e2etts_mel.h (libe2etts_mel.so): the reference's TorchSTFT.mel_spectrogram (e2e_tts/src/tools/stft.py:11-89)
on the GPU -- a recording to log-mel frames and frame energies -- and the two matrices it is loaded with.

The library loads without a GPU and ``MelFrontend(...)`` opens no device; the GPU is first touched by ``load``.  There is no CPU
fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_mel.h)
from ._lib import _addr, _expect

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_mel.so")
# the TEST build of the same source (-DE2EMEL_TEST_HOOKS: three more exports, e2emel_debug_poison_workspace, e2emel_debug_force_dense and e2emel_debug_tail), loaded instead of the product
# library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_mel_test.so")
ABI_VERSION = 1   # E2EMEL_ABI_VERSION of the include/e2etts_mel.h this binding mirrors
F32, I16 = 0, 1   # E2EMEL_F32, E2EMEL_I16
MAX_B, MAX_MEL = 4096, 1024

_P, _I, _F, _SZ, _LL = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong
# every entry point include/e2etts_mel.h declares, and all the library exports (tests/test_mel_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2emel_version": (C.c_char_p, []),
    "e2emel_abi_version": (_I, []),
    "e2emel_last_error": (C.c_char_p, [_P]),
    "e2emel_create": (_I, [_I, _I, _I, _I, C.POINTER(_P)]),
    "e2emel_destroy": (None, [_P]),
    "e2emel_load": (_I, [_P, _P, _P, _F]),
    "e2emel_stream": (_P, [_P]),
    "e2emel_order_after": (_I, [_P, _P]),
    "e2emel_sync": (_I, [_P]),
    "e2emel_device_bytes": (_SZ, [_P]),
    "e2emel_forward": (_I, [_P, _P, _I, _LL, _P, _I, _LL, _P, _P, _P, C.POINTER(_I)]),
    "e2emel_mel_dev": (_P, [_P]),
    "e2emel_energy_dev": (_P, [_P]),
    "e2emel_tile_frames": (_I, [_P]),
    "e2emel_profile_enable": (_I, [_P, _I]),
    "e2emel_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {"e2emel_debug_poison_workspace": (_I, [_P]), "e2emel_debug_force_dense": (_I, [_P, _I]),
                   "e2emel_debug_tail": (_I, [_P, _P, _P, _I, _I, _P, _P])}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree mel library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2emel", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


def hann_window(win_length: int) -> np.ndarray:
    """torch.hann_window(win_length) (periodic) in float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(win_length), dtype=np.float64) / int(win_length))


def dft_basis(n_fft: int, win_length: Optional[int] = None, window: Optional[np.ndarray] = None) -> np.ndarray:
    """[2 * bins, n_fft] float32, bins = n_fft / 2 + 1: rows 0 .. bins - 1 = w[n] cos(2 pi k n / n_fft), rows bins .. = w[n] sin(2 pi k n / n_fft),
    built in float64 and rounded once.  ``w`` is the periodic Hann window of ``win_length`` (or ``window``, any [win_length] array), centre-
    padded with zeros to n_fft as torch.stft pads a shorter window.  The angle is reduced exactly (k n mod n_fft in integers) first."""
    n_fft = int(n_fft)
    w = hann_window(n_fft if win_length is None else win_length) if window is None else np.asarray(window, np.float64).reshape(-1)
    if w.size > n_fft:
        raise ValueError(f"win_length {w.size} > n_fft {n_fft}")
    left = (n_fft - w.size) // 2
    full = np.zeros(n_fft, np.float64)
    full[left:left + w.size] = w
    bins = n_fft // 2 + 1
    kn = (np.arange(bins, dtype=np.int64)[:, None] * np.arange(n_fft, dtype=np.int64)[None, :]) % n_fft
    ang = 2.0 * np.pi * kn.astype(np.float64) / n_fft
    return np.concatenate([np.cos(ang) * full, np.sin(ang) * full], 0).astype(np.float32)


def hz_to_mel(f):
    """Slaney's auditory-toolbox scale (librosa's default, htk=False): linear, 200 / 3 Hz per mel, below 1 kHz (1 kHz = mel 15); above,
    27 mels per factor of 6.4."""
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_frequencies(n_points: int, fmin: float, fmax: float) -> np.ndarray:
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), int(n_points)))


def mel_filterbank(sr: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """[n_mels, n_fft / 2 + 1] float32 triangular filterbank: a float64 restatement of ``librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=,
    fmax=)`` as librosa 0.9.2 computes it with its defaults (Slaney scale, htk=False, norm="slaney"): n_mels + 2 points equally spaced on the
    mel scale, filter i rising from point i to point i + 1 and falling to point i + 2 over the FFT bin centres k * sr / n_fft, scaled by
    2 / (f[i + 2] - f[i]); rounded to float32 at the end.

    PARITY-UNPINNED: librosa is not installed where this project is built and tested, so this function has never been compared against
    librosa itself.  It is checked against what can be derived (tests/test_mel_host.py: the scale's fixed points, band shape, row areas).
    Every caller can pass a basis of their own instead (``MelFrontend.load``, ``models.TorchSTFT(mel_basis=...)``): with a checkpoint
    trained on librosa's matrix, pass librosa's matrix."""
    n_fft, n_mels = int(n_fft), int(n_mels)
    fmax = float(sr) / 2.0 if fmax is None else float(fmax)
    fftfreqs = np.linspace(0.0, float(sr) / 2.0, 1 + n_fft // 2)
    mel_f = mel_frequencies(n_mels + 2, float(fmin), fmax)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:n_mels] / fdiff[:n_mels, None]
    upper = ramps[2:n_mels + 2] / fdiff[1:n_mels + 1, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


def band_table(mel_basis) -> np.ndarray:
    """[n_mel, 2] int32: first and last non-zero bin of every row, (0, -1) for an all-zero row -- what e2emel_load records and the tail
    kernel sums over."""
    mb = np.asarray(mel_basis)
    out = np.zeros((mb.shape[0], 2), np.int32)
    for m, row in enumerate(mb):
        nz = np.flatnonzero(row)
        out[m] = (nz[0], nz[-1]) if nz.size else (0, -1)
    return out


def frames_of(n_valid, hop: int) -> np.ndarray:
    """mel_lens of rows with n_valid samples: floor(n_valid / hop) (reflect padding of (n_fft - hop) / 2 per side, center=False)."""
    return np.asarray(n_valid, np.int64) // int(hop)


class ResidentTensor:
    """A [shape] float32 tensor in a handle's HBM, given by its raw device address: what ``_addr`` / ``_expect`` / ``_is_cuda`` need to hand it
    to another library's entry point.  Valid until the owning handle's next forward."""
    is_cuda = True
    dtype = "float32"

    def __init__(self, ptr: int, shape):
        self.ptr, self.shape = int(ptr), tuple(int(s) for s in shape)

    def data_ptr(self) -> int:
        return self.ptr

    def is_contiguous(self) -> bool:
        return True

    def numel(self) -> int:
        return int(np.prod(self.shape))


class MelFrontend(_companion.CompanionHandle):
    """One e2emel_handle.  Inputs are numpy arrays or torch tensors (host or GPU); outputs are written into the arrays / tensors given
    (``out_*``) or returned as fresh numpy arrays when asked for by ``want``."""
    _prefix, _what, _phases = "e2emel", "mel", ("pad", "transform", "tail")

    def __init__(self, n_fft: int, hop: int, n_mel: int, device: int = 0):
        self.lib = load_library()
        self.n_fft, self.hop, self.n_mel, self.device = int(n_fft), int(hop), int(n_mel), int(device)
        h = C.c_void_p()
        rc = self.lib.e2emel_create(self.device, self.n_fft, self.hop, self.n_mel, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2emel_last_error(None).decode())
        self._h = h
        self.bins = self.n_fft // 2 + 1
        self.tile_frames = int(self.lib.e2emel_tile_frames(h))

    def load(self, dft, mel_basis, clip_val: float = 1e-5) -> None:
        """dft [2 * bins, n_fft] (``dft_basis``), mel_basis [n_mel, bins], both float32 host arrays."""
        dft = np.ascontiguousarray(dft, dtype=np.float32)
        mb = np.ascontiguousarray(mel_basis, dtype=np.float32)
        if dft.shape != (2 * self.bins, self.n_fft):
            raise ValueError(f"dft basis of shape {dft.shape}, expected {(2 * self.bins, self.n_fft)}")
        if mb.shape != (self.n_mel, self.bins):
            raise ValueError(f"mel basis of shape {mb.shape}, expected {(self.n_mel, self.bins)}")
        self._check(self.lib.e2emel_load(self._h, dft.ctypes.data, mb.ctypes.data, float(clip_val)), "e2emel_load")

    def forward(self, audio, n_valid=None, out_mel=None, out_energy=None, want=("mel", "energy")):
        """audio [B, n] float32 in [-1, 1] or int16 PCM (numpy or torch, host or GPU; rows may be strided), n_valid [B] or None
        -> dict with "T", "mel_lens" [B] int64 (numpy) and the numpy arrays named in ``want``: "mel" [B, T, n_mel] channels-last,
        "energy" [B, T].  Both stay resident (``resident()``)."""
        if audio.ndim != 2:
            raise ValueError(f"expected audio of shape [B, n], got {tuple(audio.shape)}")
        B, n = int(audio.shape[0]), int(audio.shape[1])
        is_np = isinstance(audio, np.ndarray)
        dt = audio.dtype.name if is_np else str(audio.dtype).replace("torch.", "")
        if dt not in ("float32", "int16"):
            raise TypeError(f"audio: dtype {dt}, expected float32 or int16")
        esz = 4 if dt == "float32" else 2
        if is_np:
            if audio.strides[1] != esz or (B > 1 and (audio.strides[0] % esz or audio.strides[0] < n * esz)):
                audio = np.ascontiguousarray(audio)
            stride, addr = (audio.strides[0] // esz if B > 1 else n), audio.ctypes.data
        else:
            if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n):
                audio = audio.contiguous()
            stride, addr = (audio.stride(0) if B > 1 else n), audio.data_ptr()
        if n_valid is None:
            nv = np.full(B, n, np.int64)
        else:
            nv = np.ascontiguousarray(np.asarray(n_valid.cpu() if hasattr(n_valid, "cpu") else n_valid), dtype=np.int64).reshape(-1)
            if nv.shape != (B,):
                raise ValueError(f"n_valid: {nv.size} elements, expected {B}")
        T = int(frames_of(nv, self.hop).max())   # the library's own formula; it validates n_valid and returns the same T
        r = {}
        if T >= 1:
            if out_mel is None and "mel" in want:
                out_mel = r["mel"] = np.empty((B, T, self.n_mel), np.float32)
            if out_energy is None and "energy" in want:
                out_energy = r["energy"] = np.empty((B, T), np.float32)
            _expect(out_mel, "out_mel", "float32", B * T * self.n_mel)
            _expect(out_energy, "out_energy", "float32", B * T)
        else:
            out_mel = out_energy = None   # the library refuses this call (no frame); nothing may be written
        lens = np.zeros(B, np.int64)
        t_out = C.c_int(0)
        self._order(audio, out_mel, out_energy)
        self._check(self.lib.e2emel_forward(self._h, addr, F32 if dt == "float32" else I16, stride, nv.ctypes.data, B, n, _addr(out_mel),
                                            _addr(out_energy), lens.ctypes.data, C.byref(t_out)), "e2emel_forward")
        assert t_out.value == T
        r["T"], r["mel_lens"] = T, lens
        self._resident = (B, T)
        return r

    def resident(self):
        """(mel [B, T, n_mel], energy [B, T]) of the last forward as ResidentTensor views of the handle's HBM."""
        mp, ep = self.lib.e2emel_mel_dev(self._h), self.lib.e2emel_energy_dev(self._h)
        if not mp or not ep:
            raise RuntimeError("nothing is resident (no forward has completed)")
        B, T = self._resident
        return ResidentTensor(mp, (B, T, self.n_mel)), ResidentTensor(ep, (B, T))

    def force_dense(self, on: bool = True):
        """Test build only (E2ETTS_TEST_HOOKS=1): walk all bins of every mel row instead of the recorded bands."""
        self._hook("force_dense", 1 if on else 0)

    def debug_tail(self, spec, frames):
        """Test build only (E2ETTS_TEST_HOOKS=1): the tail kernel alone on the caller's spectrum.  spec [B, T + n_overlap - 1, Cpad] float32
        (numpy; re | im | padding per row, Cpad = 2 * bins rounded up to a multiple of 32), frames [B] -> (mel [B, T, n_mel], energy [B, T])."""
        spec = np.ascontiguousarray(spec, dtype=np.float32)
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        nov, cpad = self.n_fft // self.hop, (2 * self.bins + 31) // 32 * 32
        B, T = spec.shape[0], spec.shape[1] - nov + 1
        if spec.ndim != 3 or spec.shape[2] != cpad or T < 1 or fr.shape != (B,):
            raise ValueError(f"spec of shape {spec.shape} / {fr.size} frame counts: expected [B, T + {nov - 1}, {cpad}] and [B]")
        mel, energy = np.empty((B, T, self.n_mel), np.float32), np.empty((B, T), np.float32)
        self._hook("tail", spec.ctypes.data, fr.ctypes.data, B, T, mel.ctypes.data, energy.ctypes.data)
        self._resident = (B, T)
        return mel, energy
