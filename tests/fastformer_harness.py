"""ctypes binding of the e2ekt_* entry points of tests/csrc/fastformer_harness.hip (libe2etts_kernels_test.so): launch_ff_pool with its two
shape queries and launch_ff_scale of csrc/fastformer.hip.  Device buffers are passed as `torch.Tensor.data_ptr()` integers (or None); the
launch entries return the wrapper's message (None = launched).  A wrapper that refuses returns before it launches, so the refusals work
without a GPU (the pointers are never dereferenced: pass any non-zero, suitably aligned integer for 'present')."""
from __future__ import annotations

import ctypes as C

from kernel_harness import LIB_PATH, I, P, S, SZ, _msg   # noqa: F401

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

    def bind(name, args, res=S):
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args

    bind("e2ekt_fastformer_version", [])
    bind("e2ekt_ff_pool", [P, I, P, P, P, P, P, P, SZ, I, I, I, I, P])
    bind("e2ekt_ff_scale", [P, I, P, P, P, P, I, I, I, P])
    bind("e2ekt_ff_pool_workspace_bytes", [I, I, I, I], SZ)
    bind("e2ekt_ff_pool_splits", [I, I, I, I], I)
    _lib = lib
    return lib


def version() -> str:
    return load().e2ekt_fastformer_version().decode()


def ff_pool(v, v_ld, scale, wl, bl, lens, out, ws, ws_bytes, B, N, H, head_size, stream=None):
    return _msg(load().e2ekt_ff_pool(v, v_ld, scale, wl, bl, lens, out, ws, ws_bytes, B, N, H, head_size, stream))


def ff_scale(q, q_ld, gk, x, wv, qx, B, N, H, stream=None):
    return _msg(load().e2ekt_ff_scale(q, q_ld, gk, x, wv, qx, B, N, H, stream))


def workspace_bytes(B, N, H, head_size) -> int:
    return int(load().e2ekt_ff_pool_workspace_bytes(B, N, H, head_size))


def splits(B, N, H, head_size) -> int:
    return int(load().e2ekt_ff_pool_splits(B, N, H, head_size))
