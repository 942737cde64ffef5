"""ctypes binding of libe2etts_kernels_test.so (tests/csrc/kernel_harness.hip, kernel_harness_act16.hip): the e2ekt_* entry points around the launch wrappers of
csrc/kernels.h.  Device buffers are passed as `torch.Tensor.data_ptr()` integers (or None); every launch entry returns the wrapper's
message (None = launched).  The host-only entries (conv_gemm_class, *_supported, *_bytes) work without a GPU."""
from __future__ import annotations

import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "e2e_tts_amd", "lib", "libe2etts_kernels_test.so")

P, I, F, LL, SZ, S = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t, C.c_char_p

# argument lists, in the order of the C entry points
CONV_ARGS = [("in", P), ("w", P), ("wfrag", P), ("bias", P), ("res", P), ("out", P), ("lens", P), ("act_rows", P), ("act_rows_host", P),
             ("B", I), ("T", I), ("Cin", I), ("Cout", I), ("KW", I), ("dil", I), ("pad", I), ("in_bs", LL), ("out_bs", LL), ("res_bs", LL),
             ("in_ld", I), ("out_ld", I), ("res_ld", I), ("x3", I), ("zero_tap_split", I), ("in_slope", F), ("act", I), ("act_slope", F),
             ("accumulate", I), ("out_div", F)]
CONV_DEFAULTS = dict(wfrag=None, bias=None, res=None, lens=None, act_rows=None, act_rows_host=None, KW=1, dil=1, pad=0, res_bs=0, res_ld=0,
                     x3=0, zero_tap_split=0, in_slope=1.0, act=0, act_slope=0.0, accumulate=0, out_div=1.0)
BCONV_ARGS = [("in", P), ("in_bf16", I), ("in_slope", F), ("in_add0", P), ("in_add1", P), ("in_add2", P), ("in_div", F), ("wimg", P), ("KWe", I),
              ("tap_split", I), ("bias", P), ("act_slope", F), ("res", P), ("accumulate", I), ("out_div", F), ("out", P), ("out_b", P),
              ("outb_slope", F), ("B", I), ("T", I), ("Cin", I), ("Cout", I), ("KW", I), ("dil", I), ("pad", I), ("rows_hint", I), ("act16", I)]
BCONV_DEFAULTS = dict(in_bf16=0, in_slope=1.0, in_add0=None, in_add1=None, in_add2=None, in_div=1.0, tap_split=0, bias=None, act_slope=1.0,
                      res=None, accumulate=0, out_div=1.0, out=None, out_b=None, outb_slope=1.0, dil=1, pad=0, rows_hint=0, act16=0)
PAIR_ARGS = [("x", P), ("wfrag", P), ("b1", P), ("b2", P), ("out", P), ("act_rows", P), ("act_rows_host", P), ("B", I), ("T", I), ("C", I),
             ("KW", I), ("dil", I), ("x_bs", LL), ("out_bs", LL), ("slope", F), ("accumulate", I), ("out_div", F), ("mode", I), ("bimg1", P),
             ("bimg2", P)]
PAIR_DEFAULTS = dict(wfrag=None, act_rows=None, act_rows_host=None, slope=0.1, accumulate=0, out_div=1.0, mode=1, bimg1=None, bimg2=None)
BCONV_GROUP_ARGS = [a for a in BCONV_ARGS if a[0] != "rows_hint"]       # e2ekt_conv_bf16_group: one array of n per argument
PAIR_GROUP_ARGS = [a for a in PAIR_ARGS if a[0] not in ("wfrag", "act_rows", "act_rows_host", "x_bs", "out_bs")]
RB_ARGS = [("n", I), ("x", P), ("out", P), ("bimg", P), ("b1", P), ("b2", P), ("dil", P), ("KW", P), ("accumulate", P), ("out_div", P),
           ("n_pairs", I), ("B", I), ("T", I), ("C", I), ("x_bs", LL), ("out_bs", LL), ("slope", F), ("act16", I)]
RB_MAX_PAIRS = 4

_lib = None


def _msg(r):
    return None if r is None else r.decode()


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py`")
    import torch  # noqa: F401  -- first, so that the process has ONE HIP runtime (see e2e_tts_amd/_lib.load_library)
    lib = C.CDLL(LIB_PATH)

    def bind(name, res, args):
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args

    conv, bconv, pair, rb = ([t for _, t in a] for a in (CONV_ARGS, BCONV_ARGS, PAIR_ARGS, RB_ARGS))
    bind("e2ekt_version", S, [])
    bind("e2ekt_act16_version", S, [])
    for n in ("conv_gemm", "conv_ksplit", "conv_rows"):
        bind("e2ekt_" + n, S, conv + [P])
    bind("e2ekt_conv_gemm_class", S, conv)
    bind("e2ekt_conv_ksplit_supported", I, conv)
    bind("e2ekt_conv_rows_supported", I, conv)
    bind("e2ekt_conv_bf16", S, bconv + [P])
    bind("e2ekt_conv_bf16_supported", I, bconv)
    bind("e2ekt_conv_bf16_class", S, bconv)
    bind("e2ekt_conv_bf16_group", S, [I] + [P] * len(BCONV_GROUP_ARGS) + [P])
    bind("e2ekt_pair_bf16_group", S, [I] + [P] * len(PAIR_GROUP_ARGS) + [P])
    bind("e2ekt_conv_post_bf16", S, [P, P, P, P, P, I, LL, I, I, P, I])
    bind("e2ekt_x3_frag_bytes", SZ, [I, I, I])
    bind("e2ekt_x3_to_frag", S, [P, P, I, I, I, P])
    bind("e2ekt_f32_to_frag", S, [P, P, I, I, I, P])
    bind("e2ekt_bf16_image_bytes", SZ, [I, I, I, I])
    bind("e2ekt_bf16_image", S, [P, P, I, I, I, I, P])
    bind("e2ekt_f16_image", S, [P, P, I, I, I, I, P])
    bind("e2ekt_attention", S, [P, P, P, I, I, I, I, I, P, P, P, SZ])
    bind("e2ekt_attention_workspace_bytes", SZ, [I, I, I, I])
    bind("e2ekt_attention_par_max_grid", LL, [])
    bind("e2ekt_rel_attention", S, [P, P, I, P, P, P, I, I, I, I, P, P])
    bind("e2ekt_layernorm", S, [P, P, P, P, P, I, I, I, F, P])
    bind("e2ekt_resblock_pair_supported", I, [I, I, I])
    bind("e2ekt_resblock_pair", S, pair + [P])
    bind("e2ekt_pair_bf16", S, pair + [P])
    bind("e2ekt_pair_bf16_supported", I, pair)
    bind("e2ekt_resblock_chain_supported", I, [I, I, P, I])
    bind("e2ekt_resblock_chain", S, [P, P, P, P, P, P, P, I, I, I, I, P, LL, LL, F, I, F, I, P])
    for n in ("rb_bf16_group", "rb_bf16_stage"):
        bind("e2ekt_" + n, S, rb + [P])
    bind("e2ekt_rb_bf16_supported", I, rb)
    bind("e2ekt_rb_bf16_stage_supported", I, rb)
    bind("e2ekt_conv_post", S, [P, P, P, P, P, I, LL, I, I, P, P, P, P, F])
    bind("e2ekt_dwconv_swish", S, [P, P, P, P, I, I, I, I, P])
    bind("e2ekt_dwconv_glu_swish", S, [P, P, P, P, P, I, I, I, I, P, P])
    bind("e2ekt_glu", S, [P, P, LL, I, P])
    _lib = lib
    return lib


def version() -> str:
    return load().e2ekt_version().decode()


def _flat(spec, defaults, kw):
    bad = set(kw) - {n for n, _ in spec}
    if bad:
        raise TypeError(f"unknown arguments {sorted(bad)}")
    vals = {**defaults, **kw}
    return [vals[n] for n, _ in spec]


def _keep_i32(values):
    """A host int32 array for the `*_host` arguments: returns (ctypes array, address); the caller keeps the array alive over the call."""
    arr = (C.c_int32 * len(values))(*[int(v) for v in values])
    return arr, C.addressof(arr)


def _conv_call(fn, kw, stream):
    kw = dict(kw)
    keep = None
    if kw.get("act_rows_host") is not None and not isinstance(kw["act_rows_host"], int):
        keep, kw["act_rows_host"] = _keep_i32(kw["act_rows_host"])
    a = _flat(CONV_ARGS, CONV_DEFAULTS, kw)
    r = fn(*a) if stream is False else fn(*a, stream)
    del keep
    return r


def conv_gemm(stream=None, **kw):
    return _msg(_conv_call(load().e2ekt_conv_gemm, kw, stream))


def conv_ksplit(stream=None, **kw):
    return _msg(_conv_call(load().e2ekt_conv_ksplit, kw, stream))


def conv_rows(stream=None, **kw):
    return _msg(_conv_call(load().e2ekt_conv_rows, kw, stream))


def conv_gemm_class(**kw) -> str:
    """Host only: pointers are never dereferenced except act_rows_host; pass any non-zero integer for 'present'."""
    return _conv_call(load().e2ekt_conv_gemm_class, kw, False).decode()


def conv_ksplit_supported(**kw) -> bool:
    return bool(_conv_call(load().e2ekt_conv_ksplit_supported, kw, False))


def conv_rows_supported(**kw) -> bool:
    return bool(_conv_call(load().e2ekt_conv_rows_supported, kw, False))


def conv_bf16(stream=None, **kw):
    return _msg(load().e2ekt_conv_bf16(*_flat(BCONV_ARGS, BCONV_DEFAULTS, kw), stream))


def conv_bf16_supported(**kw) -> bool:
    return bool(load().e2ekt_conv_bf16_supported(*_flat(BCONV_ARGS, BCONV_DEFAULTS, kw)))


def conv_bf16_class(**kw) -> str:
    return load().e2ekt_conv_bf16_class(*_flat(BCONV_ARGS, BCONV_DEFAULTS, kw)).decode()


def _group_call(fn, spec, defaults, members, stream):
    """One ctypes array of len(members) per argument of `spec`, in its order."""
    n = len(members)
    names = {nm for nm, _ in spec}
    bad = {k for m in members for k in m if k not in names}
    missing = {nm for m in members for nm in names if nm not in m and nm not in defaults}
    if bad or missing:
        raise TypeError(f"unknown arguments {sorted(bad)}, missing arguments {sorted(missing)}")
    keep = []
    for name, t in spec:
        vals = [{**defaults, **m}[name] for m in members]
        keep.append((t * n)(*vals))
    r = fn(n, *[C.addressof(a) for a in keep], stream)
    del keep
    return _msg(r)


def conv_bf16_group(members, stream=None):
    """members: 1 .. 4 dicts of conv_bf16's arguments (rows_hint is the group's own)."""
    return _group_call(load().e2ekt_conv_bf16_group, BCONV_GROUP_ARGS, BCONV_DEFAULTS, members, stream)


def pair_bf16_group(members, stream=None):
    """members: 1 .. 4 dicts of pair_bf16's arguments (dense tensors: x_bs = out_bs = T * C; no wfrag / act_rows)."""
    return _group_call(load().e2ekt_pair_bf16_group, PAIR_GROUP_ARGS, PAIR_DEFAULTS, members, stream)


def x3_frag_bytes(Cout, KW, Cin) -> int:
    return int(load().e2ekt_x3_frag_bytes(Cout, KW, Cin))


def bf16_image_bytes(Cout, KW, Cin, tap_split=0) -> int:
    return int(load().e2ekt_bf16_image_bytes(Cout, KW, Cin, tap_split))


def x3_to_frag(x3, frag, Cout, KW, Cin, stream=None):
    return _msg(load().e2ekt_x3_to_frag(x3, frag, Cout, KW, Cin, stream))


def f32_to_frag(w, frag, Cout, KW, Cin, stream=None):
    return _msg(load().e2ekt_f32_to_frag(w, frag, Cout, KW, Cin, stream))


def bf16_image(x3, img, Cout, KW, Cin, tap_split=0, stream=None):
    return _msg(load().e2ekt_bf16_image(x3, img, Cout, KW, Cin, tap_split, stream))


def f16_image(w, img, Cout, KW, Cin, tap_split=0, stream=None):
    return _msg(load().e2ekt_f16_image(w, img, Cout, KW, Cin, tap_split, stream))


def attention(qkv, out, lens, B, N, H, n_head, x3=0, stream=None, lens_host=None, ws=None, ws_bytes=0):
    keep = addr = None
    if lens_host is not None:
        keep, addr = _keep_i32(lens_host)
    r = load().e2ekt_attention(qkv, out, lens, B, N, H, n_head, x3, stream, addr, ws, ws_bytes)
    del keep
    return _msg(r)


def attention_workspace_bytes(B, N, H, n_head) -> int:
    return int(load().e2ekt_attention_workspace_bytes(B, N, H, n_head))


def attention_par_max_grid() -> int:
    return int(load().e2ekt_attention_par_max_grid())


def rel_attention(qkv, pos, pos_rows, u, v, out, B, N, H, n_head, stream=None, pos_x3=None):
    return _msg(load().e2ekt_rel_attention(qkv, pos, pos_rows, u, v, out, B, N, H, n_head, stream, pos_x3))


def layernorm(x, y, gamma, beta, lens, B, N, C_, eps, stream=None):
    return _msg(load().e2ekt_layernorm(x, y, gamma, beta, lens, B, N, C_, eps, stream))


def resblock_pair_supported(C_, KW, dil) -> bool:
    return bool(load().e2ekt_resblock_pair_supported(C_, KW, dil))


def _pair_call(fn, kw, stream):
    kw = dict(kw)
    keep = None
    if kw.get("act_rows_host") is not None and not isinstance(kw["act_rows_host"], int):
        keep, kw["act_rows_host"] = _keep_i32(kw["act_rows_host"])
    a = _flat(PAIR_ARGS, PAIR_DEFAULTS, kw)
    r = fn(*a) if stream is False else fn(*a, stream)
    del keep
    return r


def resblock_pair(stream=None, **kw):
    return _msg(_pair_call(load().e2ekt_resblock_pair, kw, stream))


def pair_bf16(stream=None, **kw):
    return _msg(_pair_call(load().e2ekt_pair_bf16, kw, stream))


def pair_bf16_supported(**kw) -> bool:
    return bool(_pair_call(load().e2ekt_pair_bf16_supported, kw, False))


def resblock_chain_supported(C_, KW, dil) -> bool:
    d = (C.c_int * len(dil))(*dil)
    return bool(load().e2ekt_resblock_chain_supported(C_, KW, C.addressof(d), len(dil)))


def resblock_chain(x, wfrag, b1, b2, out, B, T, C_, dil, x_bs, out_bs, KW=3, slope=0.1, accumulate=0, out_div=1.0, mode=1, act_rows=None,
                   act_rows_host=None, stream=None):
    pb1, pb2, d = (P * 3)(*b1), (P * 3)(*b2), (C.c_int * 3)(*dil)
    keep = addr = None
    if act_rows_host is not None:
        keep, addr = _keep_i32(act_rows_host)
    r = load().e2ekt_resblock_chain(x, wfrag, C.addressof(pb1), C.addressof(pb2), out, act_rows, addr, B, T, C_, KW, C.addressof(d), x_bs, out_bs,
                                    slope, accumulate, out_div, mode, stream)
    del keep
    return _msg(r)


def _rb_args(members, n_pairs, B, T, C_, x_bs, out_bs, slope, act16):
    """members: dicts with x, out, bimg [(conv1, conv2)] * n_pairs, b1, b2, dil [n_pairs], KW, accumulate, out_div."""
    n = len(members)
    x, out = (P * n)(*[m["x"] for m in members]), (P * n)(*[m["out"] for m in members])
    bimg, b1, b2 = (P * (n * RB_MAX_PAIRS * 2))(), (P * (n * RB_MAX_PAIRS))(), (P * (n * RB_MAX_PAIRS))()
    dil = (C.c_int * (n * RB_MAX_PAIRS))(*([1] * (n * RB_MAX_PAIRS)))
    for i, m in enumerate(members):
        for k in range(n_pairs):
            bimg[(i * RB_MAX_PAIRS + k) * 2], bimg[(i * RB_MAX_PAIRS + k) * 2 + 1] = m["bimg"][k]
            b1[i * RB_MAX_PAIRS + k], b2[i * RB_MAX_PAIRS + k], dil[i * RB_MAX_PAIRS + k] = m["b1"][k], m["b2"][k], m["dil"][k]
    KW = (C.c_int * n)(*[m["KW"] for m in members])
    acc = (C.c_int * n)(*[m.get("accumulate", 0) for m in members])
    div = (C.c_float * n)(*[m.get("out_div", 1.0) for m in members])
    keep = (x, out, bimg, b1, b2, dil, KW, acc, div)
    return keep, [n] + [C.addressof(a) for a in keep] + [n_pairs, B, T, C_, x_bs, out_bs, slope, act16]


def rb_bf16_group(members, n_pairs, B, T, C_, x_bs, out_bs, slope=0.1, act16=0, stream=None, stage=False):
    keep, a = _rb_args(members, n_pairs, B, T, C_, x_bs, out_bs, slope, act16)
    fn = load().e2ekt_rb_bf16_stage if stage else load().e2ekt_rb_bf16_group
    r = fn(*a, stream)
    del keep
    return _msg(r)


def rb_bf16_supported(members, n_pairs, B, T, C_, x_bs, out_bs, slope=0.1, act16=0, stage=False) -> bool:
    keep, a = _rb_args(members, n_pairs, B, T, C_, x_bs, out_bs, slope, act16)
    fn = load().e2ekt_rb_bf16_stage_supported if stage else load().e2ekt_rb_bf16_supported
    r = fn(*a)
    del keep
    return bool(r)


def conv_post(x, w, bias, wav, pcm, B, N, C_, KW, stream=None, act_rows=None, act_rows_host=None, x_add=None, x_div=1.0):
    keep = addr = None
    if act_rows_host is not None:
        keep, addr = _keep_i32(act_rows_host)
    xa = None
    if x_add is not None:
        xa = (P * 3)(*(list(x_add) + [None] * (3 - len(x_add))))
    r = load().e2ekt_conv_post(x, w, bias, wav, pcm, B, N, C_, KW, stream, act_rows, addr, C.addressof(xa) if xa is not None else None, x_div)
    del keep
    return _msg(r)


def conv_post_bf16(x, w16, bias16, wav, pcm, B, N, C_, KW, fp16=False, stream=None):
    return _msg(load().e2ekt_conv_post_bf16(x, w16, bias16, wav, pcm, B, N, C_, KW, stream, int(fp16)))


def dwconv_swish(x, w, bias, out, B, N, C_, k, stream=None):
    return _msg(load().e2ekt_dwconv_swish(x, w, bias, out, B, N, C_, k, stream))


def dwconv_glu_swish(x, w, bias, out, scratch, B, N, C_, k, stream=None):
    """Returns (message, fused): fused tells which form ran."""
    fused = C.c_int(-1)
    r = load().e2ekt_dwconv_glu_swish(x, w, bias, out, scratch, B, N, C_, k, stream, C.addressof(fused))
    return _msg(r), bool(fused.value == 1)


def glu(x, out, rows, C_, stream=None):
    return _msg(load().e2ekt_glu(x, out, rows, C_, stream))
