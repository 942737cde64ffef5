"""Shared by the teacher-forced tests (tests/test_forced_host.py, tests/test_gpu_forced.py): the fixtures of tools/make_forced_goldens.py, the
configuration and synthetic weights each was made with, and the ctypes binding of the e2ekt_* entry points of tests/csrc/forced_harness.hip."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from conftest import GOLD, ROOT
from e2e_tts_amd import config as cfgmod, synth_weights as sw

MODEL_FIXTURES = ["forced_tiny_b3", "forced_tiny_wide_b1", "forced_tiny_frame_b3", "forced_tiny_nouv_b3", "forced_tiny_partial_b3", "forced_full_b2"]
STATS = cfgmod.DEFAULT_STATS
VOC_SEED = 4321
KT_LIB = os.path.join(ROOT, "e2e_tts_amd", "lib", "libe2etts_kernels_test.so")

_G, _S = {}, {}


def load(name):
    """A fixture as a dict (cached, read-only by convention).  Missing fixtures are an error, not a skip: they are committed."""
    if name not in _G:
        _G[name] = dict(np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False))
    return _G[name]


def config_of(g):
    from oracle.make_goldens import pv_variant
    variant = str(g["variant"])
    cfg = cfgmod.default_config() if variant == "full" else cfgmod.tiny_config()
    return pv_variant(cfg, variant) if variant in ("frame", "nouv") else cfg


def states_of(g, vocoder=False):
    key = (str(g["variant"]), int(g["weight_seed"]))
    if key not in _S:
        cfg = config_of(g)
        _S[key] = [cfg, sw.make_acoustic_state(cfg, STATS, 4, seed=int(g["weight_seed"]), mode="varied"), None]
    if vocoder and _S[key][2] is None:
        _S[key][2] = sw.make_vocoder_state(_S[key][0], seed=VOC_SEED)
    return tuple(_S[key])


def targets_of(g):
    """(p_targets, e_targets) as handed to the reference's forward: frame-level [B, T]."""
    p = {"f0": g["f0"], "uv": g["uv"]} if "f0" in g else (g["pitch"] if "pitch" in g else None)
    return p, (g["energy"] if "energy" in g else None)


def bar(g, key):
    """The oracle's bar for a float array, or twice the module's own fp32-vs-float64 distance where that is larger."""
    err = float(g[key + "_err"])
    return 2.0 * err if err > 1e-5 else 1e-5


def valid_mean_l1(a, b, rows, stride=1):
    """mean |a - b| over rows t < rows[b] of [B, T, ...] arrays; `b` holds rows 0, stride, 2 stride, ... only."""
    tot, cnt = 0.0, 0
    for i, r in enumerate(rows):
        x = np.asarray(a[i, :r:stride], np.float64)
        d = np.abs(x - np.asarray(b[i, :x.shape[0]], np.float64))
        tot += float(d.sum())
        cnt += d.size
    return tot / max(cnt, 1)


_kt = None


def harness():
    global _kt
    if _kt is None:
        import torch  # noqa: F401  -- first: one HIP runtime per process (e2e_tts_amd/_lib.load_library)
        lib = C.CDLL(KT_LIB)
        P, I, F = C.c_void_p, C.c_int, C.c_float
        lib.e2ekt_forced_version.restype = C.c_char_p
        lib.e2ekt_soft_expand.restype = C.c_char_p
        lib.e2ekt_soft_expand.argtypes = [P, P, P, P, P, P, P, I, I, I, I, P]
        lib.e2ekt_teacher_scan.restype = C.c_char_p
        lib.e2ekt_teacher_scan.argtypes = [P, P, P, P, P, P, I, P, P, P, I, I, I, P]
        lib.e2ekt_target_embed.restype = C.c_char_p
        lib.e2ekt_target_embed.argtypes = [P, P, P, P, P, P, I, I, I, F, F, F, F, P, P, I, I, I, P, P, P, P, I, P]
        _kt = lib
    return _kt
