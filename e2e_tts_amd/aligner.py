"""ctypes binding of include/e2etts_align.h (libe2etts_align.so): the reference's AlignmentEncoder and monotonic alignment search
(U/layers.py:275-369, U/function.py:96-137) on the GPU, and the beta-binomial attention prior of its data loader.

The library loads without a GPU and ``Aligner(...)`` opens no device; the GPU is first touched by ``load_weights`` or by the first
call that computes.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from ._lib import _addr, _expect, _is_cuda

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_align.so")
# the TEST build of the same source (-DE2EALIGN_TEST_HOOKS: one more export, e2ealign_debug_poison_workspace), loaded instead of the product
# library only when E2ETTS_TEST_HOOKS=1 is in the environment (tests/conftest.py sets it), as _lib.py does for the main library
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_align_test.so")
ABI_VERSION = 1   # E2EALIGN_ABI_VERSION of the include/e2etts_align.h this binding mirrors
E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM = 0, -1, -2, -3, -4
LOG_MAP = 1       # E2EALIGN_LOG_MAP
MAX_ATT, MAX_L, MAX_B = 128, 2048, 4096

# every entry point include/e2etts_align.h declares, and all the library exports (tests/test_aligner_host.py compares the three)
EXPORTED_SYMBOLS = [
    "e2ealign_version", "e2ealign_abi_version", "e2ealign_last_error", "e2ealign_create", "e2ealign_destroy", "e2ealign_load_weights",
    "e2ealign_stream", "e2ealign_order_after", "e2ealign_sync", "e2ealign_device_bytes", "e2ealign_forward", "e2ealign_mas", "e2ealign_align",
    "e2ealign_profile_enable", "e2ealign_profile_read",
]
TEST_HOOK_SYMBOLS = ["e2ealign_debug_poison_workspace"]

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree alignment library (built by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    hooks = os.environ.get("E2ETTS_TEST_HOOKS", "") not in ("", "0")
    path = TEST_LIB_PATH if hooks else LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  e2e_tts_amd has no CPU fallback.")
    import torch  # noqa: F401  (ONE HIP runtime per process: see _lib.load_library)
    lib = C.CDLL(path)
    P, I, F, SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    lib.e2ealign_version.restype = C.c_char_p
    lib.e2ealign_version.argtypes = []
    lib.e2ealign_abi_version.restype = I
    lib.e2ealign_abi_version.argtypes = []
    if lib.e2ealign_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.e2ealign_abi_version()}, this binding mirrors version {ABI_VERSION}: rebuild the library")
    lib.e2ealign_last_error.restype = C.c_char_p
    lib.e2ealign_last_error.argtypes = [P]
    lib.e2ealign_create.restype = I
    lib.e2ealign_create.argtypes = [I, I, I, I, F, C.POINTER(P)]
    lib.e2ealign_destroy.restype = None
    lib.e2ealign_destroy.argtypes = [P]
    lib.e2ealign_load_weights.restype = I
    lib.e2ealign_load_weights.argtypes = [P, P, SZ]
    lib.e2ealign_stream.restype = P
    lib.e2ealign_stream.argtypes = [P]
    lib.e2ealign_order_after.restype = I
    lib.e2ealign_order_after.argtypes = [P, P]
    lib.e2ealign_sync.restype = I
    lib.e2ealign_sync.argtypes = [P]
    lib.e2ealign_device_bytes.restype = SZ
    lib.e2ealign_device_bytes.argtypes = [P]
    lib.e2ealign_forward.restype = I
    lib.e2ealign_forward.argtypes = [P, P, P, P, P, P, I, I, I, P, P]
    lib.e2ealign_mas.restype = I
    lib.e2ealign_mas.argtypes = [P, P, I, P, P, I, I, I, P, P]
    lib.e2ealign_align.restype = I
    lib.e2ealign_align.argtypes = [P, P, P, P, P, P, P, I, I, I, P, P, P, P]
    lib.e2ealign_profile_enable.restype = I
    lib.e2ealign_profile_enable.argtypes = [P, I]
    lib.e2ealign_profile_read.restype = I
    lib.e2ealign_profile_read.argtypes = [P, C.POINTER(C.c_double)]
    if hooks:
        lib.e2ealign_debug_poison_workspace.restype = I
        lib.e2ealign_debug_poison_workspace.argtypes = [P]
    _lib = lib
    return lib


def beta_binomial_prior_distribution(phoneme_count: int, mel_count: int, scaling_factor: float = 1.0) -> np.ndarray:
    """[mel_count, phoneme_count] float64 attention prior, the values the reference's data preparation computes
    (e2e_tts/src/tools/utils.py:129-139): frame i (1-based) holds the beta-binomial pmf with phoneme_count trials and shape parameters
    (s * i, s * (mel_count + 1 - i)) at 0 .. phoneme_count - 1.  One vectorised scipy call over the whole [frames, phonemes] grid."""
    from scipy.stats import betabinom
    frame = np.arange(1, int(mel_count) + 1, dtype=np.float64)[:, None]
    phoneme = np.arange(int(phoneme_count))[None, :]
    return betabinom.pmf(phoneme, int(phoneme_count), scaling_factor * frame, scaling_factor * (int(mel_count) + 1 - frame))


def pad_attn_prior(priors, max_mel_len: int, max_txt_len: int) -> np.ndarray:
    """Right zero-padded [B, max_mel_len, max_txt_len] float32 batch of per-utterance priors, as the reference's collate function builds it
    (e2e_tts/src/tools/dataloader.py:274-281: a float32 torch tensor of zeros that the float64 priors are assigned into)."""
    out = np.zeros((len(priors), int(max_mel_len), int(max_txt_len)), np.float32)
    for b, p in enumerate(priors):
        p = np.asarray(p)
        out[b, :p.shape[0], :p.shape[1]] = p
    return out


def batch_prior(txt_lens, mel_lens, max_mel_len: int, max_txt_len: int, scaling_factor: float = 1.0) -> np.ndarray:
    """The padded prior batch of rows with txt_lens[b] phonemes and mel_lens[b] frames."""
    return pad_attn_prior([beta_binomial_prior_distribution(int(p), int(m), scaling_factor) for p, m in zip(txt_lens, mel_lens)],
                          max_mel_len, max_txt_len)


class Aligner:
    """One e2ealign_handle.  Inputs are numpy arrays or torch tensors (host or GPU), outputs are written into the arrays / tensors given
    (``out_*``) or returned as fresh numpy arrays when asked for by ``want``."""

    def __init__(self, n_mel: int, n_att: int, n_text: int, temperature: float, device: int = 0):
        self.lib = load_library()
        self.n_mel, self.n_att, self.n_text, self.temperature, self.device = int(n_mel), int(n_att), int(n_text), float(temperature), int(device)
        h = C.c_void_p()
        rc = self.lib.e2ealign_create(self.device, self.n_mel, self.n_att, self.n_text, self.temperature, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2ealign_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.e2ealign_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc == E_OK:
            return
        msg = f"{what}: {self.lib.e2ealign_last_error(self._h).decode()}"
        if rc == E_INVAL:
            raise ValueError(msg)
        if rc == E_NOMEM:
            raise MemoryError(msg)
        raise RuntimeError(msg)

    def _order(self, *xs):
        """Order the handle's stream after torch's current stream when any argument lives on the GPU."""
        if any(_is_cuda(x) for x in xs):
            import torch
            with torch.cuda.device(self.device):
                s = torch.cuda.current_stream().cuda_stream
            self._check(self.lib.e2ealign_order_after(self._h, s), "e2ealign_order_after")

    def load_weights(self, blob) -> None:
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(self.lib.e2ealign_load_weights(self._h, blob.ctypes.data, blob.size), "e2ealign_load_weights")

    @staticmethod
    def _lens(x, B: int, name: str):
        if x is None:
            return None
        if not _is_cuda(x):
            x = np.ascontiguousarray(np.asarray(x), dtype=np.int64).reshape(-1)
        _expect(x, name, "int64", B)
        return x

    def forward(self, mel, keys, speaker=None, txt_lens=None, prior=None, out_attn=None, out_logprob=None, want=("attn", "attn_logprob")):
        """mel [B, T, n_mel] (channels-last), keys [B, L, n_text], speaker [B, n_text] | None, txt_lens [B] | None, prior [B, T, L] | None
        -> dict with the numpy arrays named in ``want`` (besides whatever ``out_*`` received); the maps stay resident for mas(None, ...)."""
        B, T, L = int(mel.shape[0]), int(mel.shape[1]), int(keys.shape[1])
        _expect(mel, "mel", "float32", B * T * self.n_mel)
        _expect(keys, "keys", "float32", B * L * self.n_text)
        _expect(speaker, "speaker", "float32", B * self.n_text)
        _expect(prior, "prior", "float32", B * T * L)
        txt_lens = self._lens(txt_lens, B, "txt_lens")
        r = {}
        if out_attn is None and "attn" in want:
            out_attn = r["attn"] = np.empty((B, T, L), np.float32)
        if out_logprob is None and "attn_logprob" in want:
            out_logprob = r["attn_logprob"] = np.empty((B, T, L), np.float32)
        _expect(out_attn, "out_attn", "float32", B * T * L)
        _expect(out_logprob, "out_logprob", "float32", B * T * L)
        self._order(mel, keys, speaker, txt_lens, prior, out_attn, out_logprob)
        self._check(self.lib.e2ealign_forward(self._h, _addr(mel), _addr(keys), _addr(speaker), _addr(txt_lens), _addr(prior), B, T, L,
                                              _addr(out_attn), _addr(out_logprob)), "e2ealign_forward")
        return r

    def mas(self, attn, in_lens, out_lens, B: Optional[int] = None, T: Optional[int] = None, L: Optional[int] = None, log_map: bool = False,
            out_hard=None, out_dur=None, want=("attn_hard", "dur")):
        """attn [B, T, L] probabilities (log-probabilities with ``log_map``), or None for the resident attn of the last forward (B, T, L then
        given) -> dict with "attn_hard" [B, T, L] and "dur" [B, L] float32."""
        if attn is not None:
            B, T, L = (int(v) for v in attn.shape)
            _expect(attn, "attn", "float32", B * T * L)
        in_lens, out_lens = self._lens(in_lens, B, "in_lens"), self._lens(out_lens, B, "out_lens")
        r = {}
        if out_hard is None and "attn_hard" in want:
            out_hard = r["attn_hard"] = np.empty((B, T, L), np.float32)
        if out_dur is None and "dur" in want:
            out_dur = r["dur"] = np.empty((B, L), np.float32)
        _expect(out_hard, "out_hard", "float32", B * T * L)
        _expect(out_dur, "out_dur", "float32", B * L)
        self._order(attn, in_lens, out_lens, out_hard, out_dur)
        self._check(self.lib.e2ealign_mas(self._h, _addr(attn), LOG_MAP if log_map else 0, _addr(in_lens), _addr(out_lens), B, T, L,
                                          _addr(out_hard), _addr(out_dur)), "e2ealign_mas")
        return r

    def align(self, mel, keys, speaker, txt_lens, mel_lens, prior=None, out_dur=None, out_hard=None, out_attn=None, out_logprob=None,
              want=("dur",)):
        """forward + mas in one call -> dict with the arrays of ``want`` ("dur", "attn_hard", "attn", "attn_logprob")."""
        B, T, L = int(mel.shape[0]), int(mel.shape[1]), int(keys.shape[1])
        _expect(mel, "mel", "float32", B * T * self.n_mel)
        _expect(keys, "keys", "float32", B * L * self.n_text)
        _expect(speaker, "speaker", "float32", B * self.n_text)
        _expect(prior, "prior", "float32", B * T * L)
        txt_lens, mel_lens = self._lens(txt_lens, B, "txt_lens"), self._lens(mel_lens, B, "mel_lens")
        r = {}
        if out_dur is None and "dur" in want:
            out_dur = r["dur"] = np.empty((B, L), np.float32)
        if out_hard is None and "attn_hard" in want:
            out_hard = r["attn_hard"] = np.empty((B, T, L), np.float32)
        if out_attn is None and "attn" in want:
            out_attn = r["attn"] = np.empty((B, T, L), np.float32)
        if out_logprob is None and "attn_logprob" in want:
            out_logprob = r["attn_logprob"] = np.empty((B, T, L), np.float32)
        _expect(out_dur, "out_dur", "float32", B * L)
        for x, n in ((out_hard, "out_hard"), (out_attn, "out_attn"), (out_logprob, "out_logprob")):
            _expect(x, n, "float32", B * T * L)
        self._order(mel, keys, speaker, txt_lens, mel_lens, prior, out_dur, out_hard, out_attn, out_logprob)
        self._check(self.lib.e2ealign_align(self._h, _addr(mel), _addr(keys), _addr(speaker), _addr(txt_lens), _addr(mel_lens), _addr(prior),
                                            B, T, L, _addr(out_dur), _addr(out_hard), _addr(out_attn), _addr(out_logprob)), "e2ealign_align")
        return r

    def profile_enable(self, on: bool = True):
        self._check(self.lib.e2ealign_profile_enable(self._h, 1 if on else 0), "e2ealign_profile_enable")

    def profile_read(self):
        """Milliseconds of the last call's phases: {"proj", "attn", "mas"}."""
        ms = (C.c_double * 3)()
        self._check(self.lib.e2ealign_profile_read(self._h, ms), "e2ealign_profile_read")
        return {"proj": ms[0], "attn": ms[1], "mas": ms[2]}

    def poison_workspace(self):
        """Test build only (E2ETTS_TEST_HOOKS=1)."""
        if not hasattr(self.lib, "e2ealign_debug_poison_workspace"):
            raise RuntimeError("poison_workspace needs the test build of the alignment library (E2ETTS_TEST_HOOKS=1)")
        self._check(self.lib.e2ealign_debug_poison_workspace(self._h), "e2ealign_debug_poison_workspace")

    def device_bytes(self) -> int:
        return int(self.lib.e2ealign_device_bytes(self._h))

    def sync(self):
        self._check(self.lib.e2ealign_sync(self._h), "e2ealign_sync")
