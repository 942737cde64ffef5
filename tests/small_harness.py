"""ctypes binding of the e2ekt_* entry points of tests/csrc/small_harness.hip (libe2etts_kernels_test.so): the launch wrappers of the
integer-decision and index kernels of csrc/small_kernels.hip.  Device buffers are passed as `torch.Tensor.data_ptr()` integers (or None);
every entry returns the wrapper's message (None = launched).  A wrapper that refuses returns before it launches, so the refusals work
without a GPU (the pointers are never dereferenced: pass any non-zero, suitably aligned integer for 'present')."""
from __future__ import annotations

import ctypes as C

from kernel_harness import LIB_PATH, F, I, LL, P, S, _msg   # noqa: F401

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

    bind("e2ekt_small_version", [])
    bind("e2ekt_embed", [P, P, P, P, I, I, I, I, P])
    bind("e2ekt_add_speaker", [P, P, P, P, I, I, I, I, I, P])
    bind("e2ekt_var_positions", [P, P, P, I, P, P, I, I, I, I, P])
    bind("e2ekt_rowdot", [P, P, P, P, P, I, I, I, I, P])
    bind("e2ekt_duration", [P, F, P, I, I, P, P, P, P, I, I, P])
    bind("e2ekt_variance_embed", [P, P, P, F, F, F, F, P, I, P, P, P, P, I, I, I, I, P, I, P, I, I, P, I, I, I, P, I, P])
    bind("e2ekt_length_regulate", [P, P, P, P, P, I, I, I, I, P])
    bind("e2ekt_add_positions", [P, P, I, I, I, P])
    bind("e2ekt_act_rows", [P, P, I, I, I, LL, LL, P])
    bind("e2ekt_accum_div", [P, P, P, LL, F, P])
    bind("e2ekt_transpose_bct_btc", [P, P, I, I, I, P])
    bind("e2ekt_reflect_lrelu", [P, P, I, LL, I, F, P])
    bind("e2ekt_istft", [P, I, P, P, P, P, I, LL, I, I, P])
    _lib = lib
    return lib


def version() -> str:
    return load().e2ekt_small_version().decode()


def embed(ids, emb, pos, x, B, L, H, n_rows, stream=None):
    return _msg(load().e2ekt_embed(ids, emb, pos, x, B, L, H, n_rows, stream))


def add_speaker(xin, x, spk, speaker, n_spk_ids, n_speakers, B, L, H, stream=None):
    return _msg(load().e2ekt_add_speaker(xin, x, spk, speaker, n_spk_ids, n_speakers, B, L, H, stream))


def var_positions(x, posbuf, table, table_rows, alpha, y, B, L, H, compute_positions=True, stream=None):
    return _msg(load().e2ekt_var_positions(x, posbuf, table, table_rows, alpha, y, B, L, H, int(compute_positions), stream))


def rowdot(x, w, b, out, lens, B, L, C_, O, stream=None):
    return _msg(load().e2ekt_rowdot(x, w, b, out, lens, B, L, C_, O, stream))


def duration(log_d, d_control, dur, cum, mel64, mel32, B, L, ctl=(None, 0, 0), stream=None):
    """ctl: CtlRef as (p, sb, sl)."""
    return _msg(load().e2ekt_duration(log_d, d_control, ctl[0], ctl[1], ctl[2], dur, cum, mel64, mel32, B, L, stream))


def variance_embed(x, pitch_pred, energy_pred, p_control, e_control, f0_mean, f0_std, energy_bins, n_bins, pitch_emb, energy_emb, pitch_idx,
                   energy_idx, B, L, H, pitch_mode=0, pitch_bins=None, feat=3, pctl=(None, 0, 0), ectl=(None, 0, 0), N=0, cum=None, Lp=0,
                   stream=None):
    """pctl / ectl: the two CtlRefs of VarCtl as (p, sb, sl); N, cum, Lp: its other fields."""
    return _msg(load().e2ekt_variance_embed(x, pitch_pred, energy_pred, p_control, e_control, f0_mean, f0_std, energy_bins, n_bins, pitch_emb,
                                            energy_emb, pitch_idx, energy_idx, B, L, H, pitch_mode, pitch_bins, feat, pctl[0], pctl[1], pctl[2],
                                            ectl[0], ectl[1], ectl[2], N, cum, Lp, stream))


def length_regulate(x, cum, mel_lens, pos, y, B, L, T, H, stream=None):
    return _msg(load().e2ekt_length_regulate(x, cum, mel_lens, pos, y, B, L, T, H, stream))


def add_positions(y, pos, B, T, H, stream=None):
    return _msg(load().e2ekt_add_positions(y, pos, B, T, H, stream))


def act_rows(lens, out, B, add, mul, cap, add_rows=0, stream=None):
    return _msg(load().e2ekt_act_rows(lens, out, B, add, mul, cap, add_rows, stream))


def accum_div(S_, Sj, n, div, Sk=None, stream=None):
    return _msg(load().e2ekt_accum_div(S_, Sj, Sk, n, div, stream))


def transpose_bct_btc(x, out, B, C_, T, stream=None):
    return _msg(load().e2ekt_transpose_bct_btc(x, out, B, C_, T, stream))


def reflect_lrelu(x, out, B, n, C_, slope, stream=None):
    return _msg(load().e2ekt_reflect_lrelu(x, out, B, n, C_, slope, stream))


def istft(q, ldq, specphase, ri, wav, pcm, B, F_, nfft, hop, stream=None):
    return _msg(load().e2ekt_istft(q, ldq, specphase, ri, wav, pcm, B, F_, nfft, hop, stream))
