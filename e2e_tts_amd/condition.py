"""ctypes binding of include/e2etts_condition.h (libe2etts_condition.so): what the reference does to a recording first
(modules/metrics/audio_processing.py: normalize_signal) -- set_channels, remove_silent, set_loudness -- on int16 PCM on the GPU.

pydub does these steps in integers through the standard library's audioop (rms, mul, tomono); the library reproduces that arithmetic bit
for bit (tests/golden/condition_cases.npz holds what audioop gave).  The pydub layer itself -- millisecond positions, window stepping,
range merging, the zero padding of a short slice -- is restated from its source and is UNPINNED AGAINST PYDUB (pydub is not a dependency):
the definition in the header is the contract.  Two stated deviations: a span with rms == 0 (or no samples) gets gain 1 where the
reference computes an infinite gain, and ``trim="both"`` also trims the tail, which the reference's docstring promises and its code
(``silent[-1][-1] == 0``) never does; ``trim="reference"`` reproduces the code.

The library loads without a GPU and ``Conditioner(...)`` opens no device before its first computing call.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_condition.h)
from ._lib import _addr, _expect
from .resample import ResidentAudio, _audio_layout

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_condition.so")
# the TEST build of the same source (-DE2ECOND_TEST_HOOKS: one more export, e2econd_debug_poison_workspace), loaded instead of the product
# library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_condition_test.so")
ABI_VERSION = 1   # E2ECOND_ABI_VERSION of the include/e2etts_condition.h this binding mirrors
MAX_B, MIN_RATE, MAX_RATE, MAX_W = 4096, 1000, 384000, 4096
TRIM_NONE, TRIM_REFERENCE, TRIM_BOTH = 0, 1, 2
WANT_PCM, WANT_WAV = 1, 2
TRIMS = {None: TRIM_NONE, "reference": TRIM_REFERENCE, "both": TRIM_BOTH}
# e2econd_row
ROW_DTYPE = np.dtype([("len_ms", np.int32), ("n_ranges", np.int32), ("s_ms", np.int32), ("e_ms", np.int32), ("n_out", np.int64), ("sumsq", np.uint64)])
assert ROW_DTYPE.itemsize == 32

_P, _I, _SZ, _LL = C.c_void_p, C.c_int, C.c_size_t, C.c_longlong
# every entry point include/e2etts_condition.h declares, and all the library exports (tests/test_condition_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2econd_version": (C.c_char_p, []),
    "e2econd_abi_version": (_I, []),
    "e2econd_last_error": (C.c_char_p, [_P]),
    "e2econd_create": (_I, [_I, C.POINTER(_P)]),
    "e2econd_destroy": (None, [_P]),
    "e2econd_configure": (_I, [_P, _I, _I, _I]),
    "e2econd_stream": (_P, [_P]),
    "e2econd_order_after": (_I, [_P, _P]),
    "e2econd_sync": (_I, [_P]),
    "e2econd_device_bytes": (_SZ, [_P]),
    "e2econd_downmix": (_I, [_P, _P, _LL, _I, _LL, _P, _LL]),
    "e2econd_mono_dev": (_P, [_P]),
    "e2econd_analyze": (_I, [_P, _P, _LL, _P, _I, _LL, _I, _I, _P, _P]),
    "e2econd_apply": (_I, [_P, _P, _I, _P, _P, _LL, C.POINTER(_LL)]),
    "e2econd_pcm_dev": (_P, [_P]),
    "e2econd_wav_dev": (_P, [_P]),
    "e2econd_out_stride": (_LL, [_P]),
    "e2econd_tile_starts": (_LL, [_P]),
    "e2econd_profile_enable": (_I, [_P, _I]),
    "e2econd_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {"e2econd_debug_poison_workspace": (_I, [_P])}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree conditioning library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2econd", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


# ---- the host half of the definition (double arithmetic, as pydub writes it)
def threshold_k(silence_thresh: float) -> int:
    """floor(10 ** (thresh / 20) * 32768): a window is silent iff its audioop.rms <= k.  103 at -50 dBFS."""
    return int(math.floor(10 ** (float(silence_thresh) / 20) * 32768))


def len_ms(n: int, rate: int) -> int:
    return round(1000 * (int(n) / int(rate)))


def max_ranges(n: int, rate: int, W: int) -> int:
    """The most ranges a row of n samples can have (consecutive range starts are more than W apart)."""
    starts = max(0, len_ms(n, rate) - W + 1)
    return max(1, -(-starts // (W + 1)))


def rms_of(sumsq: int, n: int) -> int:
    """audioop.rms from a sum of squares over n samples."""
    return math.isqrt(int(sumsq) // int(n)) if n else 0


def dbfs_of(rms: int) -> float:
    """pydub's AudioSegment.dBFS: 20 * math.log(rms / 32768, 10) (math.log(x, 10), not log10), -inf for rms 0."""
    return 20 * math.log(rms / 32768, 10) if rms else -math.inf


def loudness_gain(sumsq: int, n: int, target_dBFS: float) -> float:
    """set_loudness's factor 10 ** ((target - dBFS) / 20).  A span with rms 0 or no samples gets 1.0 (a stated deviation: the reference
    computes an infinite gain there)."""
    rms = rms_of(sumsq, n)
    return 10 ** ((float(target_dBFS) - dbfs_of(rms)) / 20) if rms else 1.0


class ResidentRows(ResidentAudio):
    """[B, width] rows of a handle's HBM that lie ``row_stride`` elements apart."""

    def __init__(self, ptr: int, shape, dtype: str, row_stride: int):
        super().__init__(ptr, shape, dtype)
        self.row_stride = int(row_stride)

    def is_contiguous(self) -> bool:
        return self.row_stride == self.shape[1]

    def stride(self, d: int) -> int:
        return self.row_stride if d == 0 else 1


def _lens(lens, B: int, n: int):
    if lens is None:
        return np.full(B, n, np.int64)
    nv = np.ascontiguousarray(np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens), dtype=np.int64).reshape(-1)
    if nv.shape != (B,):
        raise ValueError(f"lens: {nv.size} elements, expected {B}")
    return nv


class Conditioner(_companion.CompanionHandle):
    """One e2econd_handle for recordings at ``rate`` Hz.  Inputs are int16 numpy arrays or torch tensors, on the host or the GPU."""
    _prefix, _what, _phases = "e2econd", "condition", ("upload", "compute", "fetch")

    def __init__(self, rate: int, device: Optional[int] = 0, min_silence_len: int = 100, silence_thresh: float = -50):
        self.lib = load_library()
        self.rate, self.device, self.W, self.k = int(rate), int(device or 0), int(min_silence_len), threshold_k(silence_thresh)
        h = C.c_void_p()
        rc = self.lib.e2econd_create(self.device, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2econd_last_error(None).decode())
        self._h = h
        self._keep = None      # a device input of analyze, alive until apply has read it
        self._resident = None
        try:
            self._call("configure", self.rate, self.W, self.k)
        except Exception:
            self.close()
            raise

    @property
    def tile_starts(self) -> int:
        return int(self.lib.e2econd_tile_starts(self._h))

    @staticmethod
    def _pcm(x, what="pcm"):
        x, dt, _, B, n, stride, addr = _audio_layout(x, what)
        if dt != 1:
            raise TypeError(f"{what}: conditioning works on int16 PCM, got float32")
        return x, B, n, stride, addr

    # ---- the three entry points
    def downmix(self, stereo, fetch: bool = True):
        """stereo [B, n, 2] or [B, 2 n] interleaved int16 -> mono [B, n] int16 (numpy; None with ``fetch=False``).  The result stays
        resident (``resident_mono()``)."""
        if stereo.ndim == 3:
            if stereo.shape[2] != 2:
                raise ValueError(f"expected [B, n, 2] frames, got {tuple(stereo.shape)}")
            stereo = (np.ascontiguousarray(stereo) if isinstance(stereo, np.ndarray) else stereo.contiguous()).reshape(stereo.shape[0], -1)
        x, B, n2, stride, addr = self._pcm(stereo, "stereo")
        if n2 % 2:
            raise ValueError(f"interleaved stereo rows hold an even number of elements, got {n2}")
        n = n2 // 2
        out = np.empty((B, n), np.int16) if fetch and n else None
        self._order(x)
        self._call("downmix", addr, stride, B, n, _addr(out), n)
        self._mono = (B, n)
        return out

    def resident_mono(self):
        p = self.lib.e2econd_mono_dev(self._h)
        if not p:
            raise RuntimeError("no downmix is resident")
        return ResidentAudio(p, self._mono, "int16")

    def analyze(self, pcm, lens=None, trim=None, cap: Optional[int] = None):
        """pcm [B, n] mono int16, lens [B] or None -> dict of numpy arrays [B]: "len_ms", "n_ranges", "s_ms", "e_ms", "n_out", "sumsq"
        (uint64), and "ranges": per row the list of [start, end] in ms.  ``cap``: ranges per row to make room for (default: the most a row
        of n samples can have); a row with more raises ValueError that names the true count."""
        if trim not in TRIMS:
            raise ValueError(f"trim must be None, 'reference' or 'both' (got {trim!r})")
        x, B, n, stride, addr = self._pcm(pcm)
        nv = _lens(lens, B, n)
        cap = max_ranges(n, self.rate, self.W) if cap is None else int(cap)
        rows = np.zeros(B, ROW_DTYPE)
        ranges = np.zeros((B, max(cap, 1), 2), np.int32)
        self._order(x)
        self._keep = x
        self._check(self.lib.e2econd_analyze(self._h, addr, stride, nv.ctypes.data, B, n, TRIMS[trim], cap, rows.ctypes.data, ranges.ctypes.data), "e2econd_analyze")
        r = {f: rows[f].copy() for f in ROW_DTYPE.names}
        r["ranges"] = [ranges[b, :int(rows["n_ranges"][b])].tolist() for b in range(B)]
        self._rows = r
        return r

    def apply(self, gain, want=("pcm",), out_pcm=None, out_wav=None, out_stride: Optional[int] = None, fetch: bool = True):
        """The last analysis' kept spans times gain [B] -> dict with "width" = max n_out and the numpy arrays named in ``want``: "pcm"
        [B, width] int16, "wav" [B, width] float32 = pcm / 32768; zeros at and past a row's n_out.  ``out_pcm`` / ``out_wav``: arrays or
        tensors (host or GPU) to write instead, rows ``out_stride`` elements apart.  What is named in ``want`` or given stays resident
        (``resident()``); ``fetch=False`` computes only."""
        rows = getattr(self, "_rows", None)
        if rows is None:
            raise RuntimeError("apply without an analysis")
        B = len(rows["n_out"])
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, np.float64).reshape(-1), (B,)))
        W = int(rows["n_out"].max())
        os_ = W if out_stride is None else int(out_stride)
        r = {}
        if os_ >= W and W > 0:
            if fetch and out_pcm is None and "pcm" in want:
                out_pcm = r["pcm"] = np.empty((B, W), np.int16)
            if fetch and out_wav is None and "wav" in want:
                out_wav = r["wav"] = np.empty((B, W), np.float32)
            _expect(out_pcm, "out_pcm", "int16", (B - 1) * os_ + W, at_least=True)
            _expect(out_wav, "out_wav", "float32", (B - 1) * os_ + W, at_least=True)
        elif W == 0:
            out_pcm = out_wav = None
            r.update({k: np.zeros((B, 0), np.int16 if k == "pcm" else np.float32) for k in want if k in ("pcm", "wav")})
        bits = (WANT_PCM if out_pcm is not None or "pcm" in want else 0) | (WANT_WAV if out_wav is not None or "wav" in want else 0)
        if not bits:
            raise ValueError("want names neither 'pcm' nor 'wav'")
        self._order(out_pcm, out_wav)
        w_out = C.c_longlong(-1)
        self._check(self.lib.e2econd_apply(self._h, g.ctypes.data, bits, _addr(out_pcm), _addr(out_wav), os_, C.byref(w_out)), "e2econd_apply")
        assert w_out.value == W
        r["width"] = W
        self._resident = (B, W)
        return r

    def resident(self):
        """(pcm [B, width] int16, wav [B, width] float32) of the last apply as views of the handle's HBM (rows ``row_stride`` elements
        apart); None for the one that was not computed."""
        pp, wp, rs = self.lib.e2econd_pcm_dev(self._h), self.lib.e2econd_wav_dev(self._h), int(self.lib.e2econd_out_stride(self._h))
        if not pp and not wp:
            raise RuntimeError("nothing is resident (no apply has completed)")
        return (ResidentRows(pp, self._resident, "int16", rs) if pp else None, ResidentRows(wp, self._resident, "float32", rs) if wp else None)

    def hip_stream(self) -> int:
        return _companion.CompanionHandle.stream(self)

    def order_after_stream(self, stream: int):
        """Order this handle's stream after everything queued on ``stream`` (a raw hipStream_t, e.g. another library's)."""
        self._call("order_after", stream)

    # ---- what pydub's functions give
    def detect_silence(self, pcm, lens=None):
        """Per row the list of [start, end] in ms (pydub.silence.detect_silence with seek_step 1)."""
        return self.analyze(pcm, lens)["ranges"]

    def dbfs(self, pcm, lens=None):
        """Per row AudioSegment.dBFS over its samples (float64 [B]; -inf for rms 0)."""
        r = self.analyze(pcm, lens)
        return np.array([dbfs_of(rms_of(int(s), int(n))) for s, n in zip(r["sumsq"], r["n_out"])], np.float64)

    def normalize(self, pcm, lens=None, channels: int = 1, trim=None, loudness_dBFS: Optional[float] = None, want=("pcm",), out_pcm=None, out_wav=None):
        """set_channels, remove_silent and set_loudness of a batch: pcm [B, n] int16 (``channels=2``: [B, n, 2] or [B, 2 n] interleaved,
        lens in frames) -> dict with "pcm" / "wav" as ``want`` names them, "n_out" [B] int64, "width", "ranges" (per row, of the input)
        and "gain" [B] float64."""
        if channels not in (1, 2):
            raise ValueError(f"channels must be 1 or 2 (got {channels})")
        x = pcm
        if channels == 2:
            self.downmix(pcm, fetch=False)
            x = self.resident_mono()
        a = self.analyze(x, lens, trim)
        gain = np.ones(len(a["n_out"]), np.float64)
        if loudness_dBFS is not None:
            gain = np.array([loudness_gain(int(s), int(n), loudness_dBFS) for s, n in zip(a["sumsq"], a["n_out"])], np.float64)
        r = self.apply(gain, want, out_pcm=out_pcm, out_wav=out_wav)
        r.update(n_out=a["n_out"].astype(np.int64), ranges=a["ranges"], gain=gain)
        return r


def normalize_signal(pcm, rate: int, channels: Optional[int] = None, sr: Optional[int] = None, silence_threshold=None, loudness_dBFS: Optional[float] = None,
                     device: int = 0):
    """The reference's normalize_signal (modules/metrics/audio_processing.py) on one recording, in its order: channels, rate, silence,
    loudness.  pcm [n] int16, or [n, 2] stereo frames with ``channels=1`` -> (pcm [n_out] int16, its rate).  As in the reference any truthy
    ``silence_threshold`` means -50 dBFS.  ``sr`` goes through ``resample.Resampler``: a polyphase FIR, NOT pydub's audioop.ratecv (linear
    interpolation); see resample.py."""
    x = np.asarray(pcm)
    if x.dtype != np.int16:
        raise TypeError(f"pcm: dtype {x.dtype}, expected int16")
    if x.ndim == 2 and x.shape[1] == 1:
        x = x[:, 0]
    if x.ndim == 2 and x.shape[1] == 2:
        if channels != 1:
            raise ValueError("a stereo recording needs channels=1: conditioning works on mono")
    elif x.ndim != 1:
        raise ValueError(f"expected pcm [n] or [n, 2], got {x.shape}")
    elif channels not in (None, 1):
        raise ValueError("more channels than the recording has are out of scope")
    rate = int(rate)
    if x.ndim == 2:
        c = Conditioner(rate, device)
        try:
            x = c.downmix(x[None])[0]
        finally:
            c.close()
    if sr and int(sr) != rate:
        from .resample import Resampler
        rs = Resampler(rate, int(sr), device=device)
        try:
            r = rs.forward(x[None], want=("pcm",))
            x = r["pcm"][0, :int(r["n_out"][0])]
        finally:
            rs.close()
        rate = int(sr)
    if silence_threshold or loudness_dBFS is not None:
        c = Conditioner(rate, device, silence_thresh=-50)
        try:
            r = c.normalize(x[None], trim="reference" if silence_threshold else None, loudness_dBFS=loudness_dBFS)
            x = r["pcm"][0, :int(r["n_out"][0])]
        finally:
            c.close()
    return x, rate
