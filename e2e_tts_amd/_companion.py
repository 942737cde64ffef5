"""What the ctypes bindings of the companion libraries (aligner.py, mel.py) share: the loader and the handle's common methods.

A binding declares its C ABI as one table ``name -> (restype, argtypes)`` per build (product, test hooks): the exported-symbol lists and
the ctypes prototypes both come from it."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import _is_cuda

E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM = 0, -1, -2, -3, -4   # the same in every companion's header


def load(prefix: str, lib_path: str, test_lib_path: str, abi_version: int, signatures: dict, hook_signatures: dict) -> C.CDLL:
    """dlopen a companion library (built by __graft_entry__.build()) and bind its entry points: the test build with its hooks when
    E2ETTS_TEST_HOOKS=1 is in the environment (tests/conftest.py sets it), as _lib.py does for the main library."""
    hooks = os.environ.get("E2ETTS_TEST_HOOKS", "") not in ("", "0")
    path = test_lib_path if hooks else lib_path
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  e2e_tts_amd has no CPU fallback.")
    import torch  # noqa: F401  (ONE HIP runtime per process: see _lib.load_library)
    lib = C.CDLL(path)
    have = getattr(lib, prefix + "_abi_version")()   # int (void): ctypes' default prototype
    if have != abi_version:
        raise ImportError(f"{path}: ABI version {have}, this binding mirrors version {abi_version}: rebuild the library")
    for name, (restype, argtypes) in {**signatures, **(hook_signatures if hooks else {})}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    return lib


class CompanionHandle:
    """One handle of a companion library.  A subclass sets ``_prefix`` (the entry points' ``e2ealign`` / ``e2emel``), ``_what`` (the
    library's name in messages) and ``_phases`` (the three profiled phases), and creates ``self.lib`` / ``self._h`` / ``self.device``."""
    _prefix = _what = ""
    _phases = ()

    def _call(self, name: str, *args):
        """Entry point ``name`` on this handle, its return code checked."""
        name = f"{self._prefix}_{name}"
        self._check(getattr(self.lib, name)(self._h, *args), name)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self.lib, self._prefix + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc == E_OK:
            return
        msg = f"{what}: {getattr(self.lib, self._prefix + '_last_error')(self._h).decode()}"
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
            self._call("order_after", s)

    def stream(self) -> int:
        return int(getattr(self.lib, self._prefix + "_stream")(self._h) or 0)

    def profile_enable(self, on: bool = True):
        self._call("profile_enable", 1 if on else 0)

    def profile_read(self):
        """Milliseconds of the last call's phases, by the names in ``_phases``."""
        ms = (C.c_double * 3)()
        self._call("profile_read", ms)
        return dict(zip(self._phases, ms))

    def _hook(self, name: str, *args):
        """A test hook (test build only, E2ETTS_TEST_HOOKS=1)."""
        if not hasattr(self.lib, f"{self._prefix}_debug_{name}"):
            raise RuntimeError(f"{name} needs the test build of the {self._what} library (E2ETTS_TEST_HOOKS=1)")
        self._call("debug_" + name, *args)

    def poison_workspace(self):
        """Test build only (E2ETTS_TEST_HOOKS=1)."""
        self._hook("poison_workspace")

    def device_bytes(self) -> int:
        return int(getattr(self.lib, self._prefix + "_device_bytes")(self._h))

    def sync(self):
        self._call("sync")
