"""ctypes binding of the teacher-forced companion library libe2etts_forced.so (include/e2etts_forced.h): e2etts_acoustic_forced on an
engine of the MAIN library.  The main library's exported symbols are frozen, so the pass is exported from a library of its own that is
linked from the same objects, the engine included; it shares the engine's handle, resident results, taps and error message.  Both
libraries must come from one build: ``load_library`` compares the engine version strings and refuses a mixed pair.

`_lib.Engine.acoustic_forced` is the typed wrapper; this module holds the struct mirror and the loader."""
from __future__ import annotations

import ctypes as C
import os

from . import _companion, _lib

ABI_VERSION = 1   # E2ETTS_FORCED_ABI_VERSION of the include/e2etts_forced.h this binding mirrors
_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
LIB_PATH = os.path.join(_DIR, "libe2etts_forced.so")
TEST_LIB_PATH = os.path.join(_DIR, "libe2etts_forced_test.so")   # linked with the engine object of libe2etts_hip_test.so


class CForced(C.Structure):
    """Mirror of e2etts_forced: the optional inputs of the teacher-forced pass."""
    _fields_ = [("struct_size", C.c_uint32), ("T", C.c_int32), ("durations", C.c_void_p), ("attn_soft", C.c_void_p), ("mel_lens", C.c_void_p),
                ("f0", C.c_void_p), ("uv", C.c_void_p), ("pitch", C.c_void_p), ("energy", C.c_void_p), ("pitch_frames", C.c_int32),
                ("energy_frames", C.c_int32)]


_P, _I = C.c_void_p, C.c_int
SIGNATURES = {
    "e2etts_forced_version": (C.c_char_p, []),
    "e2etts_forced_abi_version": (_I, []),
    "e2etts_forced_engine_version": (C.c_char_p, []),
    "e2etts_acoustic_forced": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, C.POINTER(CForced), _P, _P, C.POINTER(_I), _P, _P, _P, _P, _P]),
}
EXPORTED_SYMBOLS = sorted(SIGNATURES)   # all the library exports, in its product and its test build
_lib_forced = None


def load_library() -> C.CDLL:
    global _lib_forced
    if _lib_forced is None:
        main = _lib.load_library()
        lib = _companion.load("e2etts_forced", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, {})
        mine, theirs = lib.e2etts_forced_engine_version(), main.e2etts_version()
        if mine != theirs:
            raise ImportError(f"libe2etts_forced holds the engine code of {mine.decode()!r}, the main library is {theirs.decode()!r}: the two work "
                              "on one engine object and must come from one build -- rebuild (python -c 'import __graft_entry__ as g; g.build()')")
        _lib_forced = lib
    return _lib_forced
