"""ctypes binding of include/e2etts_critic.h (libe2etts_critic.so): the eval() forward of HiFi-GAN's multi-period and multi-scale
discriminators on the GPU and the figures of the reference's V/loss.py on their outputs (feature_loss, discriminator_loss,
generator_loss) -- what a vocoder checkpoint is judged by, per row and over each row's own length.  Forward and loss values only.

The definition in the header is the contract.  The library loads without a GPU and ``Critic(...)`` opens no device before weights are
loaded.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _companion
from ._companion import E_OK, E_INVAL, E_HIP, E_STATE, E_NOMEM  # noqa: F401  (the codes of include/e2etts_critic.h)
from ._lib import _addr, _expect

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_critic.so")
# the TEST build of the same source (-DE2ECR_TEST_HOOKS: the e2ecr_debug_* entry points), loaded only when E2ETTS_TEST_HOOKS=1
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libe2etts_critic_test.so")
ABI_VERSION = 1
MAX_B, MAX_LEN, MIN_LEN = 4096, 1 << 24, 12
MAX_PERIODS, MAX_SCALES, MAX_LAYERS = 8, 4, 8
MAX_DISC, MAX_MAPS = MAX_PERIODS + MAX_SCALES, MAX_LAYERS + 1
F32, PCM16 = 0, 1
ST_LENGTHS_DIFFER, ST_ONE_SIDED = 1, 2


class CLayer(C.Structure):   # e2ecr_layer
    _fields_ = [(n, C.c_int32) for n in ("cout", "k", "stride", "groups", "pad")]


class CConfig(C.Structure):   # e2ecr_config
    _fields_ = [("n_periods", C.c_int32), ("periods", C.c_int32 * MAX_PERIODS), ("n_mpd_layers", C.c_int32), ("mpd", CLayer * MAX_LAYERS),
                ("mpd_post", CLayer), ("n_scales", C.c_int32), ("n_msd_layers", C.c_int32), ("msd", CLayer * MAX_LAYERS), ("msd_post", CLayer),
                ("slope", C.c_float), ("reserved", C.c_int32), ("workspace_cap_bytes", C.c_int64)]


RESULT_DTYPE = np.dtype([("status", "<i8"), ("n_disc", "<i8"), ("fm", "<f8", (MAX_DISC, MAX_MAPS)), ("d_real", "<f8", (MAX_DISC,)),
                         ("d_fake", "<f8", (MAX_DISC,)), ("g_fake", "<f8", (MAX_DISC,))]
                        + [(n, "<f8") for n in ("feature_loss_mpd", "feature_loss_msd", "disc_loss_mpd", "disc_loss_msd", "gen_loss_mpd", "gen_loss_msd")])

_P, _I, _SZ, _LL = C.c_void_p, C.c_int, C.c_size_t, C.c_longlong
SIGNATURES = {
    "e2ecr_version": (C.c_char_p, []),
    "e2ecr_abi_version": (_I, []),
    "e2ecr_last_error": (C.c_char_p, [_P]),
    "e2ecr_default_config": (None, [C.POINTER(CConfig)]),
    "e2ecr_create": (_I, [_I, C.POINTER(CConfig), C.POINTER(_P)]),
    "e2ecr_destroy": (None, [_P]),
    "e2ecr_load_weights": (_I, [_P, _P, _SZ]),
    "e2ecr_stream": (_P, [_P]),
    "e2ecr_order_after": (_I, [_P, _P]),
    "e2ecr_sync": (_I, [_P]),
    "e2ecr_device_bytes": (_SZ, [_P]),
    "e2ecr_run": (_I, [_P, _P, _P, _LL, _P, _P, _LL, _I, _I, _P]),
    "e2ecr_fetch_scores": (_I, [_P, _I, _I, _P, _P, C.POINTER(_LL)]),
    "e2ecr_forward": (_I, [_P, _P, _P, _I, _LL, _I]),
    "e2ecr_fetch_fmap": (_I, [_P, _I, _I, _P, _P, _P]),
    "e2ecr_profile_enable": (_I, [_P, _I]),
    "e2ecr_profile_read": (_I, [_P, C.POINTER(C.c_double)]),
}
HOOK_SIGNATURES = {
    "e2ecr_debug_poison_workspace": (_I, [_P]),
    "e2ecr_debug_grouped_conv": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, _I]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)
TEST_HOOK_SYMBOLS = list(HOOK_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree critic library (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = _companion.load("e2ecr", LIB_PATH, TEST_LIB_PATH, ABI_VERSION, SIGNATURES, HOOK_SIGNATURES)
    return _lib


def default_config() -> dict:
    """The reference's tables (V/discriminator.py, V/layers.py:72-133); a layer is (cout, k, stride, groups, pad)."""
    return {"periods": [2, 3, 5, 7, 11],
            "mpd": [(32, 5, 3, 1, 2), (128, 5, 3, 1, 2), (512, 5, 3, 1, 2), (1024, 5, 3, 1, 2), (1024, 5, 1, 1, 2)], "mpd_post": (1, 3, 1, 1, 1),
            "n_scales": 3,
            "msd": [(128, 15, 1, 1, 7), (128, 41, 2, 4, 20), (256, 41, 2, 16, 20), (512, 41, 4, 16, 20), (1024, 41, 4, 16, 20), (1024, 41, 1, 16, 20),
                    (1024, 5, 1, 1, 2)], "msd_post": (1, 3, 1, 1, 1),
            "slope": 0.1, "workspace_cap_bytes": 0}


def quarter_config() -> dict:
    """The default tables with a quarter of the channels and of the groups: every grouped layer keeps its per-group shape."""
    c = default_config()
    c["mpd"] = [(co // 4, k, s, g, p) for co, k, s, g, p in c["mpd"]]
    c["msd"] = [(co // 4, k, s, max(1, g // 4), p) for co, k, s, g, p in c["msd"]]
    return c


def disc_tables(cfg: dict):
    """[(kind, index within its state dict, layers with the post layer last)] in the library's discriminator order."""
    out = [("mpd", i, list(cfg["mpd"]) + [cfg["mpd_post"]]) for i in range(len(cfg["periods"]))]
    return out + [("msd", i, list(cfg["msd"]) + [cfg["msd_post"]]) for i in range(int(cfg["n_scales"]))]


def min_len(cfg: dict) -> int:
    return max([1] + [int(p) for p in cfg["periods"]]) + 1


def _c_config(cfg: dict) -> CConfig:
    if len(cfg["periods"]) > MAX_PERIODS or len(cfg["mpd"]) > MAX_LAYERS or len(cfg["msd"]) > MAX_LAYERS:
        raise ValueError(f"at most {MAX_PERIODS} periods and {MAX_LAYERS} layers per table")
    c = CConfig()
    c.n_periods = len(cfg["periods"])
    for i, p in enumerate(cfg["periods"]):
        c.periods[i] = int(p)
    c.n_mpd_layers, c.n_msd_layers, c.n_scales = len(cfg["mpd"]), len(cfg["msd"]), int(cfg["n_scales"])
    for i, t in enumerate(cfg["mpd"]):
        c.mpd[i] = CLayer(*map(int, t))
    for i, t in enumerate(cfg["msd"]):
        c.msd[i] = CLayer(*map(int, t))
    c.mpd_post, c.msd_post = CLayer(*map(int, cfg["mpd_post"])), CLayer(*map(int, cfg["msd_post"]))
    c.slope = float(cfg["slope"])
    c.workspace_cap_bytes = int(cfg.get("workspace_cap_bytes", 0))
    return c


def _lens(lens, B: int, name: str = "lens") -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens), dtype=np.int64).reshape(-1)
    if a.shape != (B,):
        raise ValueError(f"{name}: {a.size} elements, expected {B}")
    return a


def _samples(x, name: str):
    """[B, n] float32 or int16, C-contiguous: numpy arrays are converted (floats to float32), torch tensors must match already."""
    if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
        x = np.asarray(x)
        x = np.ascontiguousarray(x, dtype=np.int16 if x.dtype == np.int16 else np.float32)
        kind = "int16" if x.dtype == np.int16 else "float32"
    else:
        kind = str(x.dtype).replace("torch.", "")
        if kind not in ("float32", "int16"):
            raise TypeError(f"{name}: dtype {x.dtype}, expected float32 or int16")
        if not x.is_contiguous() and not hasattr(x, "row_stride"):
            x = x.contiguous()
    shp = tuple(int(s) for s in x.shape)
    if len(shp) == 3 and shp[1] == 1:   # the reference's [B, 1, T]
        x, shp = x.reshape(shp[0], shp[2]), (shp[0], shp[2])
    if len(shp) != 2:
        raise ValueError(f"{name}: expected samples of shape [B, n], got {shp}")
    return x, shp, kind


class Critic(_companion.CompanionHandle):
    """One e2ecr_handle.  ``config``: the layer tables (``default_config()``); ``load(state_mpd, state_msd)`` takes the reference's two state
    dicts.  Samples are numpy arrays or torch tensors, host or GPU, float32 in [-1, 1] or int16 PCM, [B, n] with lengths [B]."""
    _prefix, _what, _phases = "e2ecr", "critic", ("dense", "grouped", "other")

    def __init__(self, config: Optional[dict] = None, device: Optional[int] = None):
        self.lib = load_library()
        self.config = default_config() if config is None else config
        self.device = int(device or 0)
        self.tables = disc_tables(self.config)
        self.n_disc = len(self.tables)
        h = C.c_void_p()
        cc = _c_config(self.config)
        rc = self.lib.e2ecr_create(self.device, C.byref(cc), C.byref(h))
        if rc != E_OK:
            raise ValueError(self.lib.e2ecr_last_error(None).decode())
        self._h = h
        self._loaded = False
        self._states = {}   # the state dicts the mirrors of e2e_tts_amd.models were given, by family ("mpd", "msd")

    def load(self, state_mpd, state_msd):
        from .packer import pack_critic
        self.load_blob(pack_critic(state_mpd, state_msd, self.config))

    def load_blob(self, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._call("load_weights", blob.ctypes.data, blob.size)
        self._loaded = True

    def order_after_stream(self, stream: int):
        """Order this handle's stream after everything queued on ``stream`` (a raw hipStream_t, e.g. the engine's)."""
        self._call("order_after", stream)

    def hip_stream(self) -> int:
        return _companion.CompanionHandle.stream(self)

    def _side(self, x, lens, name):
        x, shp, kind = _samples(x, name)
        ln = _lens(lens, shp[0], name + "_lens")
        _expect(x, name, kind, shp[0] * shp[1])
        # rows of another library's HBM may lie further apart than they are wide (condition.ResidentRows): the row stride is what the C side takes
        return x, (shp[0], int(getattr(x, "row_stride", shp[1]))), kind, ln

    def _dicts(self, res):
        out = []
        for b in range(res.shape[0]):
            r = res[b]
            d = {"status": int(r["status"]), "lengths_differ": bool(int(r["status"]) & ST_LENGTHS_DIFFER),
                 "fm": [[float(v) for v in r["fm"][i][:len(self.tables[i][2])]] for i in range(self.n_disc)],
                 "d_real": [float(v) for v in r["d_real"][:self.n_disc]], "d_fake": [float(v) for v in r["d_fake"][:self.n_disc]],
                 "g_fake": [float(v) for v in r["g_fake"][:self.n_disc]]}
            for k in ("feature_loss_mpd", "feature_loss_msd", "disc_loss_mpd", "disc_loss_msd", "gen_loss_mpd", "gen_loss_msd"):
                d[k] = float(r[k])
            out.append(d)
        return out

    def run(self, y, y_lens, g, g_lens):
        """The fused call -> one dict per row: ``fm`` [discriminator][layer], ``d_real`` / ``d_fake`` / ``g_fake`` [discriminator],
        ``feature_loss_mpd`` / ``_msd``, ``disc_loss_*``, ``gen_loss_*``, ``status``, ``lengths_differ``."""
        y, shp, kind, ly = self._side(y, y_lens, "y")
        g, shp_g, kind_g, lg = self._side(g, g_lens, "g")
        if shp_g[0] != shp[0] or kind_g != kind:   # (the row strides may differ)
            raise ValueError(f"y and g differ: {shp} {kind} against {shp_g} {kind_g}")
        res = np.zeros(shp[0], RESULT_DTYPE)
        self._order(y, g)
        self._call("run", _addr(y), ly.ctypes.data, shp[1], _addr(g), lg.ctypes.data, shp_g[1], shp[0], PCM16 if kind == "int16" else F32, res.ctypes.data)
        self._B, self._two = shp[0], True
        return self._dicts(res)

    def scores(self, y, lens, return_scores: bool = False):
        """One-sided: per row ``d_real`` = mean (1 - D(y))^2 and ``d_fake`` = mean D(y)^2 per discriminator; with ``return_scores`` also
        ``scores``: per discriminator the row's raw scores in the reference's flattened order."""
        y, shp, kind, ly = self._side(y, lens, "y")
        res = np.zeros(shp[0], RESULT_DTYPE)
        self._order(y)
        self._call("run", _addr(y), ly.ctypes.data, shp[1], None, None, 0, shp[0], PCM16 if kind == "int16" else F32, res.ctypes.data)
        self._B, self._two = shp[0], False
        out = self._dicts(res)
        if return_scores:
            per = [self.fetch_scores(d) for d in range(self.n_disc)]
            for b, o in enumerate(out):
                o["scores"] = [p[b] for p in per]
        return out

    def fetch_scores(self, disc: int, side: int = 0):
        """The raw scores of the last call: a list of B float32 arrays."""
        n = np.zeros(self._B, np.int64)
        nmax = C.c_longlong(0)
        self._call("fetch_scores", side, disc, None, n.ctypes.data, C.byref(nmax))
        out = np.zeros((self._B, max(1, nmax.value)), np.float32)
        self._call("fetch_scores", side, disc, out.ctypes.data, None, C.byref(nmax))
        return [out[b, :int(n[b])].copy() for b in range(self._B)]

    def forward(self, x, lens):
        """The materialising call for one batch: every map stays resident for ``fmap``."""
        x, shp, kind, ln = self._side(x, lens, "x")
        self._order(x)
        self._call("forward", _addr(x), ln.ctypes.data, shp[0], shp[1], PCM16 if kind == "int16" else F32)
        self._B, self._two = shp[0], False

    def fmap(self, disc: int, layer: int):
        """(map, t): map ``layer`` of discriminator ``disc`` of the last ``forward`` in the reference's layout, [B, C, Tmax, p] (period) or
        [B, C, Tmax] (scale) float32, zeros at and past t[b]."""
        shape = np.zeros(4, np.int64)
        t = np.zeros(self._B, np.int64)
        self._call("fetch_fmap", disc, layer, None, shape.ctypes.data, t.ctypes.data)
        out = np.zeros(tuple(int(s) for s in shape), np.float32)
        self._call("fetch_fmap", disc, layer, out.ctypes.data, None, None)
        return (out if self.tables[disc][0] == "mpd" else out[..., 0]), t

    def debug_grouped_conv(self, x, lens_in, wfrag, bias, out, cin, cout, k, stride, groups, pad, slope=0.1, tm=0):
        """Test build only: the grouped kernel alone on torch GPU tensors (x [B, Tin, cin] float32, lens_in [B] int32, out [B, Tout, cout])."""
        self._order(x, lens_in, wfrag, bias, out)
        self._hook("grouped_conv", x.data_ptr(), lens_in.data_ptr(), wfrag.data_ptr(), bias.data_ptr(), out.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                   int(out.shape[1]), int(cin), int(cout), int(k), int(stride), int(groups), int(pad), float(slope), int(tm))
