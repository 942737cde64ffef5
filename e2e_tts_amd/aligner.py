"""ctypes binding of include/e2etts_align.h (libe2etts_align.so): the reference's AlignmentEncoder and monotonic alignment search
(U/layers.py:275-369, U/function.py:96-137) on the GPU, and the beta-binomial attention prior of its data loader.

The library loads without a GPU and ``Aligner(...)`` opens no device; the GPU is first touched by ``load_weights`` or by the first
call that computes.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_align.h)
from ._lib import _addr, _expect, _is_cuda

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_align.so")
# the TEST build of the same source (-DE2EALIGN_TEST_HOOKS: the e2ealign_debug_* exports of the header), loaded instead of the product
# library only when E2ETTS_TEST_HOOKS=1 is in the environment (_companion.load)
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_align_test.so")
ABI_VERSION = 2   # E2EALIGN_ABI_VERSION of the include/e2etts_align.h this binding mirrors
LOG_MAP = 1       # E2EALIGN_LOG_MAP
MAX_ATT, MAX_L, MAX_B = 128, 2048, 4096
MAX_PRIOR_SCALING = 1048576.0   # E2EALIGN_MAX_PRIOR_SCALING

_P, _I, _F, _SZ, _D = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_double
# every entry point include/e2etts_align.h declares, and all the library exports (tests/test_aligner_host.py compares the three):
# name -> (restype, argtypes)
SIGNATURES = {
    "e2ealign_version": (C.c_char_p, []),
    "e2ealign_abi_version": (_I, []),
    "e2ealign_last_error": (C.c_char_p, [_P]),
    "e2ealign_create": (_I, [_I, _I, _I, _I, _F, C.POINTER(_P)]),
    "e2ealign_destroy": (None, [_P]),
    "e2ealign_load_weights": (_I, [_P, _P, _SZ]),
    "e2ealign_stream": (_P, [_P]),
    "e2ealign_order_after": (_I, [_P, _P]),
    "e2ealign_sync": (_I, [_P]),
    "e2ealign_device_bytes": (_SZ, [_P]),
    "e2ealign_forward": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "e2ealign_mas": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P]),
    "e2ealign_align": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "e2ealign_prior": (_I, [_P, _P, _P, _I, _I, _I, _D, _P]),
    "e2ealign_forward_bb": (_I, [_P, _P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P]),
    "e2ealign_align_bb": (_I, [_P, _P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P, _P, _P]),
    "e2ealign_profile_enable": (_I, [_P, _I]),
    "e2ealign_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {"e2ealign_debug_poison_workspace": (_I, [_P]),
                   "e2ealign_debug_attention": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
                   "e2ealign_debug_attention_bb": (_I, [_P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P])}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree alignment library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2ealign", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


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


class Aligner(_companion.CompanionHandle):
    """One e2ealign_handle.  Inputs are numpy arrays or torch tensors (host or GPU), outputs are written into the arrays / tensors given
    (``out_*``) or returned as fresh numpy arrays when asked for by ``want``."""
    _prefix, _what, _phases = "e2ealign", "alignment", ("proj", "attn", "mas")

    def __init__(self, n_mel: int, n_att: int, n_text: int, temperature: float, device: int = 0):
        self.lib = load_library()
        self.n_mel, self.n_att, self.n_text, self.temperature, self.device = int(n_mel), int(n_att), int(n_text), float(temperature), int(device)
        h = C.c_void_p()
        rc = self.lib.e2ealign_create(self.device, self.n_mel, self.n_att, self.n_text, self.temperature, C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2ealign_last_error(None).decode())
        self._h = h

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

    @staticmethod
    def _device_prior(prior, txt_lens, mel_lens) -> bool:
        """True for ``prior="device"`` (the beta-binomial prior generated inside the attention pass), which needs both length arrays."""
        if not isinstance(prior, str):
            return False
        if prior != "device":
            raise ValueError(f"prior must be None, a [B, T, L] array, or 'device' (got {prior!r})")
        if txt_lens is None or mel_lens is None:
            raise ValueError("prior='device' needs txt_lens and mel_lens")
        return True

    def prior(self, txt_lens, mel_lens, T: int, L: int, scaling_factor: float = 1.0, out=None):
        """The padded beta-binomial prior batch [B, T, L] float32 of rows with txt_lens[b] phonemes and mel_lens[b] frames -- what
        ``batch_prior`` computes with scipy on the host -- generated on the device (e2ealign_prior; the definition stands in
        include/e2etts_align.h: the reference's P trials evaluated at 0 .. P - 1, so rows do not sum to 1).  Written into ``out``
        (numpy array or torch tensor, host or GPU) and returned; a fresh numpy array without one."""
        B, T, L = (int(txt_lens.numel()) if _is_cuda(txt_lens) else int(np.asarray(txt_lens).size)), int(T), int(L)
        txt_lens, mel_lens = self._lens(txt_lens, B, "txt_lens"), self._lens(mel_lens, B, "mel_lens")
        if out is None:
            out = np.empty((B, T, L), np.float32)
        _expect(out, "out", "float32", B * T * L)
        self._order(txt_lens, mel_lens, out)
        self._check(self.lib.e2ealign_prior(self._h, _addr(txt_lens), _addr(mel_lens), B, T, L, float(scaling_factor), _addr(out)), "e2ealign_prior")
        return out

    def forward(self, mel, keys, speaker=None, txt_lens=None, prior=None, out_attn=None, out_logprob=None, want=("attn", "attn_logprob"),
                mel_lens=None, prior_scaling: float = 1.0):
        """mel [B, T, n_mel] (channels-last), keys [B, L, n_text], speaker [B, n_text] | None, txt_lens [B] | None, prior [B, T, L] | None |
        "device" (the beta-binomial prior of ``prior()`` for txt_lens, ``mel_lens`` and ``prior_scaling``, generated inside the attention
        pass: the same bits, no [B, T, L] prior in memory)
        -> dict with the numpy arrays named in ``want`` (besides whatever ``out_*`` received); the maps stay resident for mas(None, ...)."""
        B, T, L = int(mel.shape[0]), int(mel.shape[1]), int(keys.shape[1])
        _expect(mel, "mel", "float32", B * T * self.n_mel)
        _expect(keys, "keys", "float32", B * L * self.n_text)
        _expect(speaker, "speaker", "float32", B * self.n_text)
        gen = self._device_prior(prior, txt_lens, mel_lens)
        if gen:
            prior = None
        _expect(prior, "prior", "float32", B * T * L)
        txt_lens, mel_lens = self._lens(txt_lens, B, "txt_lens"), self._lens(mel_lens, B, "mel_lens")
        r = {}
        if out_attn is None and "attn" in want:
            out_attn = r["attn"] = np.empty((B, T, L), np.float32)
        if out_logprob is None and "attn_logprob" in want:
            out_logprob = r["attn_logprob"] = np.empty((B, T, L), np.float32)
        _expect(out_attn, "out_attn", "float32", B * T * L)
        _expect(out_logprob, "out_logprob", "float32", B * T * L)
        self._order(mel, keys, speaker, txt_lens, prior, out_attn, out_logprob)
        if gen:
            self._check(self.lib.e2ealign_forward_bb(self._h, _addr(mel), _addr(keys), _addr(speaker), _addr(txt_lens), _addr(mel_lens),
                                                     float(prior_scaling), B, T, L, _addr(out_attn), _addr(out_logprob)), "e2ealign_forward_bb")
            return r
        self._check(self.lib.e2ealign_forward(self._h, _addr(mel), _addr(keys), _addr(speaker), _addr(txt_lens), _addr(prior), B, T, L,
                                              _addr(out_attn), _addr(out_logprob)), "e2ealign_forward")
        return r

    def debug_attention(self, q, k, prior=None, txt_lens=None, want=("attn", "attn_logprob")):
        """Test build only (E2ETTS_TEST_HOOKS=1), next to poison_workspace: the attention pass of forward() alone on projections given by the
        caller, q [B, T, n_att] and k [B, L, n_att] float32 (no weights needed) -> dict with "attn" and "attn_logprob" [B, T, L]."""
        B, T, L = int(q.shape[0]), int(q.shape[1]), int(k.shape[1])
        _expect(q, "q", "float32", B * T * self.n_att)
        _expect(k, "k", "float32", B * L * self.n_att)
        _expect(prior, "prior", "float32", B * T * L)
        txt_lens = self._lens(txt_lens, B, "txt_lens")
        r = {name: np.empty((B, T, L), np.float32) for name in want}
        self._order(q, k, prior, txt_lens)
        self._hook("attention", _addr(q), _addr(k), _addr(prior), _addr(txt_lens), B, T, L, _addr(r.get("attn")), _addr(r.get("attn_logprob")))
        return r

    def debug_attention_bb(self, q, k, txt_lens, mel_lens, scaling_factor: float = 1.0, want=("attn", "attn_logprob")):
        """Test build only: ``debug_attention`` with the generated prior of ``forward(..., prior="device")``."""
        B, T, L = int(q.shape[0]), int(q.shape[1]), int(k.shape[1])
        _expect(q, "q", "float32", B * T * self.n_att)
        _expect(k, "k", "float32", B * L * self.n_att)
        txt_lens, mel_lens = self._lens(txt_lens, B, "txt_lens"), self._lens(mel_lens, B, "mel_lens")
        r = {name: np.empty((B, T, L), np.float32) for name in want}
        self._order(q, k, txt_lens, mel_lens)
        self._hook("attention_bb", _addr(q), _addr(k), _addr(txt_lens), _addr(mel_lens), float(scaling_factor), B, T, L, _addr(r.get("attn")),
                   _addr(r.get("attn_logprob")))
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
              want=("dur",), prior_scaling: float = 1.0):
        """forward + mas in one call -> dict with the arrays of ``want`` ("dur", "attn_hard", "attn", "attn_logprob").  ``prior="device"``:
        as for ``forward``, with this call's mel_lens."""
        B, T, L = int(mel.shape[0]), int(mel.shape[1]), int(keys.shape[1])
        _expect(mel, "mel", "float32", B * T * self.n_mel)
        _expect(keys, "keys", "float32", B * L * self.n_text)
        _expect(speaker, "speaker", "float32", B * self.n_text)
        gen = self._device_prior(prior, txt_lens, mel_lens)
        if gen:
            prior = None
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
        if gen:
            self._check(self.lib.e2ealign_align_bb(self._h, _addr(mel), _addr(keys), _addr(speaker), _addr(txt_lens), _addr(mel_lens),
                                                   float(prior_scaling), B, T, L, _addr(out_dur), _addr(out_hard), _addr(out_attn),
                                                   _addr(out_logprob)), "e2ealign_align_bb")
            return r
        self._check(self.lib.e2ealign_align(self._h, _addr(mel), _addr(keys), _addr(speaker), _addr(txt_lens), _addr(mel_lens), _addr(prior),
                                            B, T, L, _addr(out_dur), _addr(out_hard), _addr(out_attn), _addr(out_logprob)), "e2ealign_align")
        return r
