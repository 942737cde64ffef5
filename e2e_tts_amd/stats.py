"""ctypes binding of include/e2etts_stats.h (libe2etts_stats.so): the corpus statistics of the reference's ``TextMelLoader.build_stats``
(src/tools/dataloader.py:106-151) -- ``stats.json`` -- from frame values that lie on the GPU, and the data loader's energy target.

The definition in the header is the contract: per utterance the reference's IQR outlier rule with numpy's float32 percentile arithmetic,
bit for bit; the mean and std of what is kept merged over the corpus in double by Chan's update in row order (within a double sum's
rounding of sklearn's ``partial_fit``, whose own bits depend on the order the files were visited in); min and max of the normalised
values over all frames.

The library loads without a GPU and ``CorpusStats(...)`` opens no device before something is added.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Mapping, Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_stats.h)
from ._lib import _addr, _expect, _is_cuda

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_stats.so")
# the TEST build of the same source (-DE2EST_TEST_HOOKS: two more exports, the e2est_debug_* entry points), loaded instead of the
# product library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_stats_test.so")
ABI_VERSION = 1   # E2EST_ABI_VERSION of the include/e2etts_stats.h this binding mirrors
MAX_B, MAX_ROW = 4096, 16384
F0, ENERGY, PITCH = 0, 1, 2          # E2EST_F0, E2EST_ENERGY, E2EST_PITCH
KIND_NAMES = ("f0", "energy", "pitch")

ROW_DTYPE = np.dtype([("n", "<i8"), ("n_kept", "<i8"), ("sum", "<f8"), ("mean", "<f8"), ("m2", "<f8"), ("p25", "<f4"), ("p75", "<f4"), ("lower", "<f4"),
                      ("upper", "<f4"), ("min", "<f4"), ("max", "<f4"), ("status", "<i4"), ("reserved", "<i4")])      # e2est_row
BLOCK_DTYPE = np.dtype([(n, "<i8") for n in ("present", "rows", "n_frames", "n_kept")]
                       + [(n, "<f8") for n in ("mean", "std", "m2", "min", "max", "raw_min", "raw_max")])             # e2est_block

_P, _I, _SZ, _LL, _D = C.c_void_p, C.c_int, C.c_size_t, C.c_int64, C.c_double
# every entry point include/e2etts_stats.h declares, and all the library exports (tests/test_stats_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2est_version": (C.c_char_p, []),
    "e2est_abi_version": (_I, []),
    "e2est_last_error": (C.c_char_p, [_P]),
    "e2est_create": (_I, [_I, C.POINTER(_P)]),
    "e2est_destroy": (None, [_P]),
    "e2est_stream": (_P, [_P]),
    "e2est_order_after": (_I, [_P, _P]),
    "e2est_sync": (_I, [_P]),
    "e2est_device_bytes": (_SZ, [_P]),
    "e2est_reset": (_I, [_P]),
    "e2est_add": (_I, [_P, _I, _P, _LL, _P, _I, _I]),
    "e2est_fetch_rows": (_I, [_P, _P]),
    "e2est_result": (_I, [_P, _P]),
    "e2est_normalize": (_I, [_P, _P, _LL, _P, _I, _I, _D, _D, _P]),
    "e2est_profile_enable": (_I, [_P, _I]),
    "e2est_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {
    "e2est_debug_poison_workspace": (_I, [_P]),
    "e2est_debug_sorted": (_I, [_P, _P, _LL, _P, _I, _I, _P]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree statistics library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2est", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


def bins(stats: Mapping[str, object], n: int = 255):
    """(pitch bins or None, energy bins): ``linspace(min, max, n)`` of a block's normalised range, float32 -- what the model's constructor
    builds for its quantisers (the reference's ``torch.linspace(stats[...]["min"], stats[...]["max"], n_bins - 1)``)."""
    def one(name):
        if name not in stats:
            return None
        return np.linspace(np.float64(stats[name]["min"]), np.float64(stats[name]["max"]), int(n)).astype(np.float32)
    return one("pitch"), one("energy")


def _lens(lens, B: int) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens), dtype=np.int64).reshape(-1)
    if a.shape != (B,):
        raise ValueError(f"lens: {a.size} elements, expected {B}")
    return a


class CorpusStats(_companion.CompanionHandle):
    """One e2est_handle: three running accumulators (f0, energy, pitch) over everything added since the last ``reset``.

    ``add`` takes rows [B, T] float32 as torch tensors on the GPU, as ``ResidentTensor`` views of another library's HBM (the mel
    front-end's energy, the pitch tracker's f0) or as numpy arrays, which are uploaded.  It enqueues and returns; ``rows`` and ``result``
    wait for the device."""
    _prefix, _what, _phases = "e2est", "stats", ("rows", "merge", "normalize")

    def __init__(self, device: Optional[int] = None):
        self.lib = load_library()
        self.device = int(device or 0)
        h = C.c_void_p()
        rc = self.lib.e2est_create(self.device, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2est_last_error(None).decode())
        self._h = h
        self._last = None    # (kind, B) of the last add
        self._keep = []      # uploaded tensors an enqueued add still reads; dropped when the stream has drained

    def order_after_stream(self, stream: int):
        """Order this handle's stream after everything queued on ``stream`` (a raw hipStream_t, e.g. another library's)."""
        self._call("order_after", stream)

    def hip_stream(self) -> int:
        return _companion.CompanionHandle.stream(self)

    def reset(self):
        self._call("reset")
        self._last = None

    def _rows_arg(self, x, name):
        """-> (what holds the memory, address, row stride, B, T) of rows [B, T] float32 on the device; numpy is uploaded."""
        if x is None:
            return None
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            import torch
            a = np.ascontiguousarray(x, dtype=np.float32)
            if a.ndim != 2:
                raise ValueError(f"{name}: expected rows [B, T], got shape {a.shape}")
            x = torch.from_numpy(a).to(torch.device("cuda", self.device))
        shp = tuple(int(s) for s in x.shape)
        if len(shp) != 2:
            raise ValueError(f"{name}: expected rows [B, T], got shape {shp}")
        if str(x.dtype).replace("torch.", "") != "float32":
            raise TypeError(f"{name}: dtype {x.dtype}, expected float32")
        if not _is_cuda(x):
            import torch
            x = x.to(torch.device("cuda", self.device))
        stride = shp[1]
        if hasattr(x, "stride"):                       # a torch view whose rows are dense is read where it lies
            if shp[1] > 1 and x.stride(1) != 1:
                x = x.contiguous()
            stride = int(x.stride(0)) if shp[0] > 1 else shp[1]
            if stride < shp[1]:
                x = x.contiguous()
                stride = shp[1]
        return x, x.data_ptr(), stride, shp[0], shp[1]

    def sync(self):
        super().sync()
        self._keep.clear()

    def _hold(self, t):
        """Keeps a tensor an enqueued call still reads alive (a caller's tensor too: it may be a temporary); the list is emptied whenever
        the stream has drained, which this forces once it holds 32."""
        if len(self._keep) >= 32:
            self.sync()
        self._keep.append(t)

    def add(self, energy=None, f0=None, pitch=None, lens=None):
        """Accumulates one batch: any of ``energy``, ``f0``, ``pitch`` as rows [B, T] float32 with ``lens`` [B] frames (each in
        [1, min(T, MAX_ROW)]).  ``f0`` in Hz with 0 = unvoiced.  Bad shapes and lengths raise ValueError before anything is enqueued; a
        non-finite value is found on the device and raises at the next ``rows`` / ``result``."""
        if lens is None:
            raise ValueError("lens is required")
        given = [(k, n, x) for k, n, x in ((F0, "f0", f0), (ENERGY, "energy", energy), (PITCH, "pitch", pitch)) if x is not None]
        if not given:
            raise ValueError("nothing to add: give energy, f0 or pitch")
        for kind, name, x in given:
            t, addr, stride, B, T = self._rows_arg(x, name)
            ln = _lens(lens, B)
            self._order(t)
            self._hold(t)
            self._call("add", kind, addr, stride, ln.ctypes.data, B, T)
            self._last = (kind, B)

    def rows(self) -> np.ndarray:
        """The per-row records of the last add (``ROW_DTYPE``: n, n_kept, sum, mean, m2, p25, p75, lower, upper, min, max, status)."""
        if self._last is None:
            raise RuntimeError("rows before an add")
        out = np.zeros(self._last[1], ROW_DTYPE)
        try:
            self._call("fetch_rows", out.ctypes.data)
        finally:
            self._keep.clear()
        return out

    def blocks(self) -> np.ndarray:
        """The three e2est_block records (``BLOCK_DTYPE``), by kind: with ``n_kept``, ``mean`` and ``m2`` two ranks' accumulators merge by
        the header's formula."""
        out = np.zeros(3, BLOCK_DTYPE)
        try:
            self._call("result", out.ctypes.data)
        finally:
            self._keep.clear()
        return out

    def result(self) -> dict:
        """The dict of ``stats.json``, all Python floats: ``{"f0": {mean, std}, "energy": {max, min, mean, std}, "pitch": {...}}`` with a
        block for every kind that was added.  There is a ``"pitch"`` block only if pitch tracks were added: the engine reads only
        ``stats["f0"]`` and takes its bins from the checkpoint, so a file without ``"pitch"`` serves a ``use_uv`` model."""
        b = self.blocks()
        out = {}
        if b["present"][F0]:
            out["f0"] = {"mean": float(b["mean"][F0]), "std": float(b["std"][F0])}
        for kind in (PITCH, ENERGY):
            if b["present"][kind]:
                out[KIND_NAMES[kind]] = {k: float(b[k][kind]) for k in ("max", "min", "mean", "std")}
        return out

    def save(self, path) -> dict:
        """Writes ``result()`` as JSON (the reference's stats.json) -> the dict."""
        r = self.result()
        with open(path, "w") as f:
            json.dump(r, f, indent=4)
        return r

    def normalize(self, values, lens, mean: float, std: float, out=None):
        """The data loader's target of frame values [B, T]: ``(v - float32(mean)) / float32(std)`` in float32, 0 beyond each length (lens in
        [0, T]) -> ``out`` [B, T] float32 on the GPU (a fresh torch tensor when not given).  Enqueued on this handle's stream: order a
        consumer after ``hip_stream()``."""
        import torch
        t, addr, stride, B, T = self._rows_arg(values, "values")
        ln = _lens(lens, B)
        if out is None:
            out = torch.empty((B, T), dtype=torch.float32, device=torch.device("cuda", self.device))
        _expect(out, "out", "float32", B * T)
        if not _is_cuda(out):
            raise ValueError("out must be on the GPU")
        self._order(t, out)
        self._hold(t)
        self._call("normalize", addr, stride, ln.ctypes.data, B, T, float(mean), float(std), _addr(out))
        return out

    def add_recordings(self, model, wavs, wav_lens, wav_rate=None, condition=None):
        """One batch of recordings through ``model.recording_features`` (condition, resampler, mel front-end, pitch tracker): the
        front-end's resident frame energies and the tracker's resident f0 are added where they lie, this handle's stream ordered after
        theirs.  -> mel_lens [B] int64."""
        fe, trk, mel_lens = model.recording_features(wavs, wav_lens, wav_rate=wav_rate, condition=condition)
        self.order_after_stream(fe.stream())
        self.add(energy=fe.resident()[1], lens=mel_lens)
        self.order_after_stream(trk.hip_stream())
        self.add(f0=trk.resident(), lens=mel_lens)
        self.sync()     # the front-end and the tracker may overwrite what was read at their next forward
        self._keep.clear()
        return mel_lens

    def sorted_rows(self, values, lens) -> np.ndarray:
        """Test build only (E2ETTS_TEST_HOOKS=1): the row kernel's sorted rows [B, T] (NaN beyond each length)."""
        t, addr, stride, B, T = self._rows_arg(values, "values")
        ln = _lens(lens, B)
        out = np.full((B, T), np.nan, np.float32)
        self._order(t)
        self._hook("sorted", addr, stride, ln.ctypes.data, B, T, out.ctypes.data)
        return out

    def poison_workspace(self):
        super().poison_workspace()
        self._last = None
