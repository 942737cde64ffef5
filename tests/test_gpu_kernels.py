"""Kernel-level differential tests (-m gpu): the launch wrappers of csrc/kernels.h, called one kernel at a time through
libe2etts_kernels_test.so (tests/kernel_harness.py), every output element against a float64 reference of the same operation
(tests/kernel_ref.py) at the shapes where tiles, chunks and masks end (tests/kernel_cases.py).

Buffers.  Every device buffer is a view into a larger allocation with NaN guard bands before and after it; rows are padded (row stride >
channels) with NaN in the gaps; outputs are pre-filled with a sentinel.  After a launch the bands and gaps must hold their bits, every
element the contract says is written must be finite and inside the bars, every element it says is left alone must hold the sentinel.
An access outside a buffer but inside the band is therefore caught by value; nothing here relies on a fault.

Rows past act_rows: the kernels skip whole TILES past act_rows[b]; the rows of the last tile past it may be written (with the value the
padded launch gives them).  So rows < act_rows[b] are judged by the bars, rows >= act_rows[b] rounded up to the row tile of the kernel that
runs must hold the sentinel, and the rows between must hold either.  The same goes for conv_post's 256-sample blocks and for the query blocks of
attention under lens_host.

16-bit activations (precisions "bf16_act" / "fp16_act": launch_conv_bf16 with act16, launch_pair_bf16 in modes 3 / 4, launch_conv_post_bf16).
A 16-bit output leaves no room for an error bar, so these are judged in two tiers (tests/kernel_ref.py, last section).  Exact tier: inputs
from dyadic grids whose partial sums are exact in float32 in any order -- the output must equal the restatement bit for bit, on every
element.  General tier: Gaussian data under an interval rule (each output between the epilogue of ref - bar and of ref + bar, no element
excluded) and an aggregate rule (the share of elements that differ from the epilogue of fl32(ref), against 4 x the float32 yardstick's
share plus one element).  The fused forms are tied to that reference bit for bit: pair = two convolutions, rb = three pairs, stage = rb's."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kernel_cases as kc   # noqa: E402
import kernel_ref as kr     # noqa: E402

pytestmark = pytest.mark.gpu

BAND = 1024                       # guard band, elements (a multiple of 4: 16-byte alignment of the view is kept)
SENTINEL = np.float32(-12345.5)
RESULTS_ENV = "E2ETTS_KERNEL_TEST_RESULTS"   # optional: a JSON-lines file the tests append their figures to
_T0 = time.time()


def record(family, **kv):
    path = os.environ.get(RESULTS_ENV)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(family=family, **{k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in kv.items()})) + "\n")


@pytest.fixture(scope="module")
def kh():
    import torch
    assert torch.cuda.is_available(), "the kernel tests need the GPU"
    import kernel_harness
    import __graft_entry__ as g
    assert g.built_harness_hash() == g.harness_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    assert g.built_harness_act16_hash() == g.harness_act16_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    kernel_harness.load()
    return kernel_harness


class Guarded:
    """A [B, T, C] array (row stride ld >= C, batch stride T * ld) inside a device allocation with NaN bands and NaN gaps."""

    def __init__(self, data=None, shape=None, ld=None, dtype=np.float32, sentinel=None):
        import torch
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype
        shape = tuple(int(s) for s in shape)
        if len(shape) == 1:
            shape = (1, 1) + shape
        elif len(shape) == 2:
            shape = (1,) + shape
        self.shape = shape
        B, T, C = shape
        self.ld = ld = int(ld or C)
        n = B * T * ld
        isf = np.dtype(dtype).kind == "f"
        host = np.full(2 * BAND + n, np.nan if isf else (np.iinfo(dtype).max if np.dtype(dtype).kind == "u" else -1), dtype)   # 0xFFFF: a NaN in bf16 and fp16
        body = host[BAND:BAND + n].reshape(B, T, ld)
        body[:, :, :C] = data.reshape(shape) if data is not None else sentinel
        self.host = host
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + BAND * host.itemsize

    def fetch(self):
        """(logical [B, T, C] array, True when every element outside it -- bands and gaps -- still holds its bits)."""
        import torch
        torch.cuda.synchronize()
        back = self.dev.cpu().numpy()
        B, T, C = self.shape
        u = np.uint32 if back.itemsize == 4 else np.uint16
        same = back.view(u) == self.host.view(u)
        inside = np.zeros(back.shape, bool)
        inside[BAND:BAND + B * T * self.ld].reshape(B, T, self.ld)[:, :, :C] = True
        body = back[BAND:BAND + B * T * self.ld].reshape(B, T, self.ld)[:, :, :C]
        return body, bool(np.all(same | inside))

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        back = self.dev.cpu().numpy()
        u = np.uint32 if back.itemsize == 4 else np.uint16
        return bool(np.array_equal(back.view(u), self.host.view(u)))

    def initial(self):
        B, T, C = self.shape
        return self.host[BAND:BAND + B * T * self.ld].reshape(B, T, self.ld)[:, :, :C]


def bits_equal(a, b):
    return np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)


def i32(values):
    import torch
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------- convolutions
class ConvRig:
    """Device buffers of one (case, mode): made once, used by conv_gemm and the other convolution kernels that support the launch."""

    def __init__(self, kh, c, x3):
        self.kh, self.c, self.x3 = kh, c, x3
        self.d = d = kr.conv_data(c)
        Cout, KW, Cin = c["Cout"], c["KW"], c["Cin"]
        self.x = Guarded(d["x"], ld=Cin + c["in_pad"])
        wimg = d["w"].reshape(Cout, KW * Cin) if x3 == 0 else kr.pack_x3(d["w"])
        self.w = Guarded(wimg)
        self.frag = self.frag32 = None
        if c["wfrag"]:
            self.frag = Guarded(shape=(kh.x3_frag_bytes(Cout, KW, Cin) // 4,), sentinel=SENTINEL)
            msg = (kh.f32_to_frag if x3 == 0 else kh.x3_to_frag)(self.w.ptr, self.frag.ptr, Cout, KW, Cin)
            assert msg is None, msg
            _, ok = self.frag.fetch()
            assert ok, "the fragment image maker wrote outside its buffer"
            self.frag.host = self.frag.dev.cpu().numpy().copy()     # from here on an input: the launches must leave it as it is
        self.bias = Guarded(d["bias"]) if c["bias"] else None
        self.res = Guarded(d["res"], ld=Cout + c["res_pad"]) if c["res"] else None
        self.lens = i32(c["lens"]) if c["lens"] is not None else None
        self.rows = i32(c["act_rows"]) if c["act_rows"] is not None else None
        self.ref = kr.conv_reference(c, d, x3)
        self.yard = kr.conv_yardstick(c, d, x3, self.ref) if self.ref["linear"] and c["B"] * c["T"] * Cout >= kr.AGG_MIN_ELEMS else None

    def args(self, out):
        c = self.c
        T = c["T"]
        return dict(**{"in": self.x.ptr}, w=self.w.ptr, wfrag=self.frag.ptr if self.frag else None, bias=self.bias.ptr if self.bias else None,
                    res=self.res.ptr if self.res else None, out=out.ptr, lens=self.lens.data_ptr() if self.lens is not None else None,
                    act_rows=self.rows.data_ptr() if self.rows is not None else None,
                    act_rows_host=c["act_rows"] if (c["act_rows"] is not None and c["host"]) else None,
                    B=c["B"], T=T, Cin=c["Cin"], Cout=c["Cout"], KW=c["KW"], dil=c["dil"], pad=c["pad"], in_bs=T * self.x.ld, out_bs=T * out.ld,
                    res_bs=T * self.res.ld if self.res else 0, in_ld=self.x.ld, out_ld=out.ld, res_ld=self.res.ld if self.res else 0, x3=self.x3,
                    zero_tap_split=c["zts"], in_slope=c["in_slope"], act=c["act"], act_slope=c["act_slope"], accumulate=int(c["accumulate"]),
                    out_div=c["out_div"])

    def row_tile(self, what):
        """Rows per tile of the kernel that runs: conv_gemm's by its choice (kernel_cases.variant), conv_ksplit 32, conv_rows 128."""
        if what == "conv_gemm":
            c = self.c
            v = kc.variant(c, self.x3, 1 if c["env"] == "wg1" else 24, c["env"] != "frag64")[1]
            return int(v["tile"].split("x")[0])
        return {"conv_ksplit": 32, "conv_rows": 128}.get(what, 256)

    def run(self, fn, what):
        """Launch, then judge the whole output buffer; returns the logical result."""
        c, d = self.c, self.d
        out = Guarded(d["old"], ld=c["Cout"] + c["out_pad"]) if c["accumulate"] else Guarded(shape=(c["B"], c["T"], c["Cout"]), ld=c["Cout"] + c["out_pad"],
                                                                                                sentinel=SENTINEL)
        msg = fn(**self.args(out))
        assert msg is None, (what, msg)
        got, guard_ok = out.fetch()
        assert guard_ok, f"{what}: wrote outside the output rows (guard band or row gap changed)"
        for g in (self.x, self.w, self.bias, self.res, self.frag):
            assert g is None or g.unchanged(), f"{what}: an input buffer changed"
        computed, untouched = kr.written_mask(c, self.row_tile(what))
        r = kr.check_conv(c, d, self.x3, got, self.ref, self.yard, rows=computed)
        print(f"{what} {c['name']} x3={self.x3}: worst err/bar {r['elem_ratio']:.3g}, aggregate ratio {r['agg_ratio']}, yardstick {r['yard']}, dev {self.ref['dev']:.3g}")
        record("conv", kernel=what, case=c["name"], x3=self.x3, elem=r["elem_ratio"], agg=r["agg_ratio"], dev=self.ref["dev"], act=c["act"])
        assert r["ok"], (what, c["name"], self.x3, r["why"])
        init = out.initial()
        assert np.all(bits_equal(got[untouched], init[untouched])), f"{what}: rows past act_rows were written"
        between = ~computed & ~untouched
        if np.any(between):
            err = np.abs(got.astype(np.float64) - self.ref["ref"])[between]
            assert np.all(np.all(bits_equal(got[between], init[between]), -1) | np.all(err <= self.ref["bar"][between], -1)), \
                f"{what}: a row of the last tile past act_rows holds neither the sentinel nor the padded launch's value"
        return got, computed


def conv_case_body(kh, c):
    for x3 in kc.modes_of(c):
        rig = ConvRig(kh, c, x3)
        got, computed = rig.run(kh.conv_gemm, "conv_gemm")
        if c["act"] in kr.TRANSCENDENTAL:
            # the aggregate bar belongs to the linear part: the same launch on the same data (the generator is seeded by the name) with the
            # activation switched off.  tanh and swish are run-time branches of the same instantiation; ACT_GELU has instantiations of its own,
            # whose linear part is therefore held to the per-element bar alone
            ConvRig(kh, dict(c, act=kc.ACT_NONE), x3).run(kh.conv_gemm, "conv_gemm")
        if kc.ksplit_ok(c, x3):
            rig.run(kh.conv_ksplit, "conv_ksplit")          # its own fixed reduction order: the bars, not conv_gemm's bits
        if kc.rows_ok(c, x3):
            rows, _ = rig.run(kh.conv_rows, "conv_rows")
            assert np.all(bits_equal(rows[computed], got[computed])), f"conv_rows differs from conv_gemm ({c['name']}, x3 = {x3}): kernels.h promises the same bits"


@pytest.mark.parametrize("c", [c for c in kc.CONV_CASES if c["env"] is None], ids=lambda c: c["name"])
def test_conv_gemm_ksplit_rows(kh, c):
    conv_case_body(kh, c)


@pytest.mark.parametrize("c", kc.BCONV_CASES, ids=lambda c: c["name"])
def test_conv_bf16(kh, c):
    """conv_bf16 against float64 (the plain-bf16 operand model), and bit for bit against conv_gemm in mode 2 on the same buffers."""
    rig = ConvRig(kh, c, 2)
    Cout, KW, Cin = c["Cout"], c["KW"], c["Cin"]
    img = Guarded(shape=(kh.bf16_image_bytes(Cout, KW, Cin, c["zts"]) // 4,), sentinel=SENTINEL)
    assert kh.bf16_image(rig.w.ptr, img.ptr, Cout, KW, Cin, c["zts"]) is None
    assert img.fetch()[1]
    act_slope = {kc.ACT_NONE: 1.0, kc.ACT_RELU: 0.0, kc.ACT_LRELU: c["act_slope"]}[c["act"]]

    def bconv(**a):
        return kh.conv_bf16(**{"in": a["in"]}, in_slope=a["in_slope"], wimg=img.ptr, KWe=2 if c["zts"] else KW, tap_split=c["zts"], bias=a["bias"],
                            act_slope=act_slope, res=a["res"], accumulate=a["accumulate"], out_div=a["out_div"], out=a["out"], B=a["B"], T=a["T"], Cin=Cin,
                            Cout=Cout, KW=KW, dil=a["dil"], pad=a["pad"])

    got, computed = rig.run(bconv, "conv_bf16")
    gemm, _ = rig.run(kh.conv_gemm, "conv_gemm")
    assert np.all(bits_equal(got, gemm)), "conv_bf16 differs from conv_gemm in mode 2: kernels.h promises the same bits"


@pytest.mark.parametrize("group", ["wg1", "frag64"])
def test_conv_gemm_env_variants_in_a_child_process(kh, group):
    """E2ETTS_WG_PER_CU=1 (the persistent multi-tile loop: tpb >= 2, tile counts tpb does not divide) and E2ETTS_FRAG64=0 (the 64 x 64 tile
    on the LDS weight tile) are read once per process: a child runs those cases, one child after the other, each under its own timeout."""
    env = dict(os.environ, **kc.ENV_OF[group])
    rr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", group], env=env, capture_output=True, text=True, timeout=600)
    print(rr.stdout[-4000:])
    assert rr.returncode == 0, (rr.stdout[-3000:], rr.stderr[-3000:])
    assert f"child {group} ok" in rr.stdout


# ---------------------------------------------------------------- attention
def att_rows(c):
    """(judged [B, N], zero, sentinel): query rows < lens[b]; rows that must be 0; rows that must keep the sentinel (lens_host)."""
    B, N = c["B"], c["N"]
    lens = np.full(B, N) if c["lens"] is None else np.asarray(c["lens"])
    t = np.arange(N)[None, :]
    valid = t < lens[:, None]
    if not c["host"]:
        return valid, ~valid, np.zeros((B, N), bool)
    up = lambda q: ((lens + q - 1) // q * q)[:, None]    # noqa: E731
    return valid, ~valid & (t < up(64)), t >= up(256)


@pytest.mark.parametrize("c", kc.ATT_CASES, ids=lambda c: c["name"])
def test_attention(kh, c):
    d = kr.att_data(c)
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    H = nh * dk
    ref = kr.att_reference(c, d)
    qkv = Guarded(d["qkv"])
    lens = i32(c["lens"]) if c["lens"] is not None else None
    valid, zero, keep = att_rows(c)
    for x3 in (0, 1):
        o, W, dev = kr.att_bar(c, d, x3, ref)
        outs = []
        for use_ws in ((False, True) if c["ws"] and x3 == 0 else (False,)):
            out = Guarded(shape=(B, N, H), sentinel=SENTINEL)
            ws = None
            nbytes = kh.attention_workspace_bytes(B, N, H, nh)
            if use_ws:
                ws = Guarded(shape=(nbytes // 4,), sentinel=SENTINEL)
            msg = kh.attention(qkv.ptr, out.ptr, lens.data_ptr() if lens is not None else None, B, N, H, nh, x3,
                               lens_host=c["lens"] if c["host"] else None, ws=ws.ptr if ws else None, ws_bytes=nbytes if ws else 0)
            assert msg is None, msg
            got, guard_ok = out.fetch()
            assert guard_ok and qkv.unchanged() and (ws is None or ws.fetch()[1])
            ok, worst = kr.check_att(got, o, W, dev, valid)
            print(f"attention {c['name']} x3={x3} ws={use_ws}: float32 deviation {dev:.3g} (relative to sum p |v|), worst err/bar {worst:.3g}")
            record("attention", case=c["name"], x3=x3, ws=use_ws, dev=dev, elem=worst, sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])
            assert ok, (c["name"], x3, use_ws, worst)
            assert np.all(got[zero] == 0), "query rows >= lens[b] must be written as 0"
            assert np.all(got[keep] == SENTINEL), "query rows past the last block must keep their contents under lens_host"
            between = ~valid & ~zero & ~keep
            assert np.all((got[between] == 0) | (got[between] == SENTINEL))
            outs.append(got)
        if len(outs) == 2:
            assert N > 32 * 8, "the workspace cases have at least two key segments"
            assert np.all(bits_equal(outs[0], outs[1])), "parallel key segments differ from the in-register merge: kernels.h promises the same bits"


def att_outputs_without_workspace(kh):
    """{"<case>/<x3>": out [B, N, H]} of every ATT_CASES entry at a head dim that has a split form, in both precisions, without workspace."""
    outs = {}
    for c in kc.ATT_CASES:
        if c["dk"] not in kc.ATT_SPLIT_DK:
            continue
        B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
        qkv = Guarded(kr.att_data(c)["qkv"])
        lens = i32(c["lens"]) if c["lens"] is not None else None
        for x3 in (0, 1):
            out = Guarded(shape=(B, N, nh * dk), sentinel=SENTINEL)
            msg = kh.attention(qkv.ptr, out.ptr, lens.data_ptr() if lens is not None else None, B, N, nh * dk, nh, x3,
                               lens_host=c["lens"] if c["host"] else None, ws=None, ws_bytes=0)
            assert msg is None, msg
            got, guard_ok = out.fetch()
            assert guard_ok and qkv.unchanged(), (c["name"], x3)
            outs[f"{c['name']}/{x3}"] = got
    return outs


def test_attention_serial_form_gives_the_split_forms_bits(kh, tmp_path):
    """Per head dimension and per precision: the split form (two wavefronts per query tile, half the head dimension each; what the launcher
    takes by default) and the one-wavefront form (attention_kernel<dk>, attention_x3_kernel<dk, 8>) give the same bits on every query row
    < lens[b], and both write 0 on the rows that must be 0.  The one-wavefront form is read once per process (E2ETTS_ATT_SPLIT_MAX=0), so a
    child runs it and hands its outputs over in a file.  (b40_n257_dk64 in split precision is above the launcher's grid limit and takes the
    one-wavefront form in this process too: that comparison is trivial.)"""
    mine = att_outputs_without_workspace(kh)
    path = str(tmp_path / "att_serial.npz")
    env = dict(os.environ, **kc.ENV_OF["att_serial"])
    rr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "att_serial", path], env=env, capture_output=True, text=True, timeout=600)
    assert rr.returncode == 0, (rr.stdout[-3000:], rr.stderr[-3000:])
    assert "child att_serial ok" in rr.stdout
    theirs = np.load(path)
    assert sorted(theirs.files) == sorted(mine) and len(mine) == 2 * sum(c["dk"] in kc.ATT_SPLIT_DK for c in kc.ATT_CASES)
    assert {c["dk"] for c in kc.ATT_CASES} >= set(kc.ATT_SPLIT_DK)
    for c in kc.ATT_CASES:
        if c["dk"] not in kc.ATT_SPLIT_DK:
            continue
        valid, zero, _ = att_rows(c)
        for x3 in (0, 1):
            split, serial = mine[f"{c['name']}/{x3}"], theirs[f"{c['name']}/{x3}"]
            assert np.all(bits_equal(split[valid], serial[valid])), f"{c['name']} x3 = {x3}: the one-wavefront form differs from the split form"
            assert np.all(split[zero] == 0) and np.all(serial[zero] == 0), f"{c['name']} x3 = {x3}: query rows >= lens[b] must be written as 0"


@pytest.mark.parametrize("c", kc.REL_CASES, ids=lambda c: c["name"])
def test_rel_attention(kh, c):
    from e2e_tts_amd import packer
    d = kr.rel_data(c)
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    H = nh * dk
    qkv, pos, u, v = Guarded(d["qkv"]), Guarded(d["pos"]), Guarded(d["u"]), Guarded(d["v"])
    px = Guarded(packer.split_rows_x3(d["pos"])) if dk in kc.REL_X3_DK else None
    for x3 in ((False, True) if px is not None else (False,)):
        o, W, dev = kr.rel_bar(c, d, x3)
        out = Guarded(shape=(B, N, H), sentinel=SENTINEL)
        msg = kh.rel_attention(qkv.ptr, pos.ptr, c["pos_rows"], u.ptr, v.ptr, out.ptr, B, N, H, nh, pos_x3=px.ptr if x3 else None)
        assert msg is None, msg
        got, guard_ok = out.fetch()
        assert guard_ok and all(g.unchanged() for g in (qkv, pos, u, v)) and (px is None or px.unchanged())
        ok, worst = kr.check_att(got, o, W, dev)
        print(f"rel_attention {c['name']} x3={x3}: float32 deviation {dev:.3g}, worst err/bar {worst:.3g}")
        record("rel_attention", case=c["name"], x3=int(x3), dev=dev, elem=worst, sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])
        assert ok, (c["name"], x3, worst)


@pytest.mark.parametrize("c", kc.LN_CASES, ids=lambda c: c["name"])
def test_layernorm(kh, c):
    d = kr.ln_data(c)
    y, bar = kr.ln_reference(c, d)
    x, g, b = Guarded(d["x"]), Guarded(d["gamma"]), Guarded(d["beta"])
    out = Guarded(shape=d["x"].shape, sentinel=SENTINEL)
    lens = i32(c["lens"]) if c["lens"] is not None else None
    msg = kh.layernorm(x.ptr, out.ptr, g.ptr, b.ptr, lens.data_ptr() if lens is not None else None, c["B"], c["N"], c["C"], d["eps"])
    assert msg is None, msg
    got, guard_ok = out.fetch()
    assert guard_ok and x.unchanged() and g.unchanged() and b.unchanged()
    err = np.abs(got.astype(np.float64) - y)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err == 0, 0, np.inf))))
    print(f"layernorm {c['name']}: worst err/bar {ratio:.3g}")
    record("layernorm", case=c["name"], elem=ratio)
    assert np.all(np.isfinite(got)) and ratio <= 1.0, ratio
    assert np.all(got[0, 0] == d["beta"]) or c["lens"] is not None and c["lens"][0] == 0     # a row of constant value: (x - mean) is exactly 0


# ---------------------------------------------------------------- small kernels
@pytest.mark.parametrize("c", kc.POST_CASES, ids=lambda c: c["name"])
def test_conv_post(kh, c):
    B, N, C, KW = c["B"], c["N"], c["C"], c["KW"]
    t = np.arange(N)[None, :]
    rows = np.clip(np.asarray(c["act_rows"]), 0, N)[:, None] if c["act_rows"] is not None else np.full((B, 1), N)
    computed, untouched = (t < rows)[:, :], t >= (rows + 255) // 256 * 256
    for small in (False, True):
        d = kr.post_data(c, small)
        wav_ref, bar, dev = kr.post_reference(c, d)
        xs = [Guarded(x) for x in d["xs"]]
        w, bias = Guarded(d["w"]), Guarded(d["bias"])
        wav = Guarded(shape=(1, B, N), sentinel=SENTINEL)
        pcm = Guarded(shape=(1, B, N), dtype=np.int16, sentinel=np.int16(-7777))
        ar = i32(c["act_rows"]) if c["act_rows"] is not None else None
        msg = kh.conv_post(xs[0].ptr, w.ptr, bias.ptr, wav.ptr, pcm.ptr, B, N, C, KW, act_rows=ar.data_ptr() if ar is not None else None,
                           act_rows_host=c["act_rows"] if c["host"] else None, x_add=[x.ptr for x in xs[1:]] or None, x_div=c["x_div"])
        assert msg is None, msg
        gw, ok_w = wav.fetch()
        gp, ok_p = pcm.fetch()
        gw, gp = gw[0], gp[0]
        assert ok_w and ok_p and all(x.unchanged() for x in xs) and w.unchanged() and bias.unchanged()
        err = np.abs(gw.astype(np.float64) - wav_ref)
        worst = float(np.max(err[computed] / bar[computed]))
        assert np.all(np.isfinite(gw[computed])) and worst <= 1.0, worst
        assert np.all(gw[untouched] == SENTINEL) and np.all(gp[untouched] == -7777), "samples past act_rows were written"
        between = ~computed & ~untouched
        assert np.all((gw[between] == SENTINEL) | (err[between] <= bar[between]))
        assert np.array_equal(gp[computed], kr.pcm_of(gw)[computed]), "pcm is not (int16)(int32)(wav * 32768) of the kernel's own wav"
        excluded = 0.0
        if small:   # the reference's PCM: equal off the rounding boundaries, within 1 LSB everywhere; the excluded share is counted
            near = kr.pcm_boundary(wav_ref, bar)
            ref_pcm = np.trunc(wav_ref * 32768.0).astype(np.int32)
            diff = np.abs(gp.astype(np.int32) - ref_pcm)
            excluded = float(near[computed].mean()) if np.any(computed) else 0.0
            assert excluded <= 1e-3, excluded
            assert np.all(diff[computed & ~near] == 0) and np.all(diff[computed] <= 1), int(diff[computed].max())
        print(f"conv_post {c['name']} small={small}: tanh deviation {dev:.3g}, worst err/bar {worst:.3g}, excluded share {excluded:.3g}")
        record("conv_post", case=c["name"], small=small, dev=dev, elem=worst, excluded=excluded)


@pytest.mark.parametrize("c", kc.DW_CASES, ids=lambda c: c["name"])
def test_dwconv(kh, c):
    """dwconv_swish against float64; dwconv_glu_swish (fused where a fused form exists, else its fallback) bit for bit against glu followed by
    dwconv_swish, whose result is judged against float64 on the GLU output it read."""
    B, N, C, k = c["B"], c["N"], c["C"], c["k"]
    d = kr.dw_data(c)
    ref, bar, dev = kr.dw_reference(c, d["x"], d["w"], d["bias"])
    x, w, bias = Guarded(d["x"]), Guarded(d["w"]), Guarded(d["bias"])
    out = Guarded(shape=(B, N, C), sentinel=SENTINEL)
    assert kh.dwconv_swish(x.ptr, w.ptr, bias.ptr, out.ptr, B, N, C, k) is None
    got, ok = out.fetch()
    assert ok and x.unchanged()
    worst = float(np.max(np.abs(got.astype(np.float64) - ref) / bar))
    assert np.all(np.isfinite(got)) and worst <= 1.0, worst
    # GLU in front
    dg = kr.dw_data(c, glu=True)
    xg = Guarded(dg["x"])
    wg, bg = Guarded(dg["w"]), Guarded(dg["bias"])
    mid = Guarded(shape=(B, N, C), sentinel=SENTINEL)
    assert kh.glu(xg.ptr, mid.ptr, B * N, C) is None
    gm, ok = mid.fetch()
    gref, gbar, gdev = kr.glu_reference(dg["x"])
    worst_g = float(np.max(np.abs(gm.astype(np.float64) - gref) / np.maximum(gbar, 1e-300)))
    assert ok and np.all(np.isfinite(gm)) and worst_g <= 1.0, worst_g
    two = Guarded(shape=(B, N, C), sentinel=SENTINEL)
    assert kh.dwconv_swish(mid.ptr, wg.ptr, bg.ptr, two.ptr, B, N, C, k) is None
    g2, ok = two.fetch()
    ref2, bar2, dev2 = kr.dw_reference(c, gm, dg["w"], dg["bias"])
    worst2 = float(np.max(np.abs(g2.astype(np.float64) - ref2) / bar2))
    assert ok and worst2 <= 1.0, worst2
    one, scratch = Guarded(shape=(B, N, C), sentinel=SENTINEL), Guarded(shape=(B, N, C), sentinel=SENTINEL)
    msg, fused = kh.dwconv_glu_swish(xg.ptr, wg.ptr, bg.ptr, one.ptr, scratch.ptr, B, N, C, k)
    assert msg is None, msg
    g1, ok = one.fetch()
    assert ok and xg.unchanged() and scratch.fetch()[1]
    assert fused == kc.DW_FUSED(C, k), (fused, C, k)
    assert fused == scratch.unchanged(), "the fused form must not touch the scratch buffer; the fallback goes through it"
    assert np.all(bits_equal(g1, g2)), "dwconv_glu_swish differs from glu + dwconv_swish: kernels.h promises the same bits"
    print(f"dwconv {c['name']}: swish deviation {dev:.3g}, worst err/bar {worst:.3g} / after GLU {worst2:.3g}; glu deviation {gdev:.3g}, worst {worst_g:.3g}; fused {fused}")
    record("dwconv", case=c["name"], dev=dev, elem=max(worst, worst2), glu_dev=gdev, glu_elem=worst_g, fused=fused)


@pytest.mark.parametrize("c", kc.GLU_CASES, ids=lambda c: c["name"])
def test_glu(kh, c):
    x = (kr.rng_of(c["name"]).standard_normal((c["rows"], 2 * c["C"]), np.float32) * 3).astype(np.float32)
    ref, bar, dev = kr.glu_reference(x)
    xin, out = Guarded(x), Guarded(shape=(c["rows"], c["C"]), sentinel=SENTINEL)
    assert kh.glu(xin.ptr, out.ptr, c["rows"], c["C"]) is None
    got, ok = out.fetch()
    worst = float(np.max(np.abs(got[0].astype(np.float64) - ref) / np.maximum(bar, 1e-300)))
    record("glu", case=c["name"], dev=dev, elem=worst)
    assert ok and xin.unchanged() and np.all(np.isfinite(got)) and worst <= 1.0, worst


# ---------------------------------------------------------------- fused ResBlocks
def _pair_weights(name, C, KW, n):
    r = kr.rng_of(name)
    return [dict(w1=(r.standard_normal((C, KW, C)) / np.sqrt(KW * C)).astype(np.float32), w2=(r.standard_normal((C, KW, C)) / np.sqrt(KW * C)).astype(np.float32),
                 b1=(0.1 * r.standard_normal(C)).astype(np.float32), b2=(0.1 * r.standard_normal(C)).astype(np.float32)) for _ in range(n)]


def _images(kh, ws, mode, C, KW):
    """(weights as ConvParams::w, contiguous fragment images, bf16 images) of a list of [C, KW, C] tensors."""
    flat = [Guarded(w.reshape(C, KW * C) if mode == 0 else kr.pack_x3(w)) for w in ws]
    per = kh.x3_frag_bytes(C, KW, C) // 4
    frag = Guarded(shape=(per * len(ws),), sentinel=SENTINEL)
    for i, f in enumerate(flat):
        assert (kh.f32_to_frag if mode == 0 else kh.x3_to_frag)(f.ptr, frag.ptr + 4 * per * i, C, KW, C) is None
    bimg = []
    if mode == 2:
        for f in flat:
            g = Guarded(shape=(kh.bf16_image_bytes(C, KW, C) // 4,), sentinel=SENTINEL)
            assert kh.bf16_image(f.ptr, g.ptr, C, KW, C) is None
            bimg.append(g)
    assert frag.fetch()[1]
    return flat, frag, per, bimg


def _compose_pair(kh, x, out, flat1, flat2, b1, b2, B, T, C, KW, dil, mode, slope, accumulate, out_div, frag1=None, frag2=None):
    """The pair as two conv_gemm launches: h = c1(lrelu(x)) + b1; out = [out_old +] c2(lrelu(h)) + b2 + x [/ out_div]."""
    h = Guarded(shape=(B, T, C), sentinel=SENTINEL)
    common = dict(B=B, T=T, Cin=C, Cout=C, KW=KW, in_bs=T * C, out_bs=T * C, in_ld=C, out_ld=C, x3=mode, in_slope=slope)
    assert kh.conv_gemm(**{"in": x}, w=flat1.ptr, wfrag=frag1, bias=b1.ptr, out=h.ptr, dil=dil, pad=dil * (KW - 1) // 2, **common) is None
    assert kh.conv_gemm(**{"in": h.ptr}, w=flat2.ptr, wfrag=frag2, bias=b2.ptr, res=x, res_bs=T * C, res_ld=C, out=out, dil=1, pad=(KW - 1) // 2,
                        accumulate=int(accumulate), out_div=out_div, **common) is None
    return h


@pytest.mark.parametrize("c", kc.PAIR_CASES, ids=lambda c: c["name"])
def test_resblock_pair_is_the_composition_of_its_convolutions(kh, c):
    """launch_resblock_pair (modes 0, 1, 2) and launch_pair_bf16 (mode 2) bit for bit against two conv_gemm launches at the same shape --
    launches of the kind test_conv_gemm_ksplit_rows holds to float64 -- and, in modes 0 and 1, against the float64 composite with the bar
    propagated through the second convolution: sum |w2| bar1 + gamma S2."""
    B, T, C, KW, dil = c["B"], c["T"], c["C"], c["KW"], c["dil"]
    assert kh.resblock_pair_supported(C, KW, dil)
    r = kr.rng_of(c["name"])
    xh = r.standard_normal((B, T, C), np.float32)
    old = r.standard_normal((B, T, C), np.float32)
    pw = _pair_weights(c["name"] + "_w", C, KW, 1)[0]
    for mode in (0, 1, 2):
        x = Guarded(xh)
        flat, frag, per, bimg = _images(kh, [pw["w1"], pw["w2"]], mode, C, KW)
        b1, b2 = Guarded(pw["b1"]), Guarded(pw["b2"])
        mk = lambda: Guarded(old) if c["accumulate"] else Guarded(shape=(B, T, C), sentinel=SENTINEL)   # noqa: E731
        comp = mk()
        _compose_pair(kh, x.ptr, comp.ptr, flat[0], flat[1], b1, b2, B, T, C, KW, dil, mode, 0.1, c["accumulate"], c["out_div"],
                      frag.ptr, frag.ptr + 4 * per)
        want, ok = comp.fetch()
        assert ok
        fused = mk()
        msg = kh.resblock_pair(x=x.ptr, wfrag=frag.ptr, b1=b1.ptr, b2=b2.ptr, out=fused.ptr, B=B, T=T, C=C, KW=KW, dil=dil, x_bs=T * C, out_bs=T * C,
                               slope=0.1, accumulate=int(c["accumulate"]), out_div=c["out_div"], mode=mode)
        assert msg is None, msg
        got, ok = fused.fetch()
        assert ok and x.unchanged() and np.all(np.isfinite(got))
        assert np.all(bits_equal(got, want)), f"resblock_pair mode {mode} differs from its two convolutions: kernels.h promises the same bits"
        if mode == 2:
            pa = dict(x=x.ptr, wfrag=frag.ptr, b1=b1.ptr, b2=b2.ptr, B=B, T=T, C=C, KW=KW, dil=dil, x_bs=T * C, out_bs=T * C, slope=0.1,
                      accumulate=int(c["accumulate"]), out_div=c["out_div"], mode=2, bimg1=bimg[0].ptr, bimg2=bimg[1].ptr)
            bp = mk()
            assert kh.pair_bf16_supported(out=bp.ptr, **pa)
            assert kh.pair_bf16(out=bp.ptr, **pa) is None
            gb, ok = bp.fetch()
            assert ok and np.all(bits_equal(gb, want)), "pair_bf16 differs from resblock_pair in mode 2: kernels.h promises the same bits"
        else:   # the float64 composite
            c1 = kc._case("p1", B, T, C, C, KW, dil, bias=True, in_slope=0.1)
            d1 = dict(x=xh, w=pw["w1"], bias=pw["b1"], res=None, old=None)
            r1 = kr.conv_reference(c1, d1, mode)
            c2 = kc._case("p2", B, T, C, C, KW, 1, bias=True, res=True, in_slope=0.1, accumulate=c["accumulate"], out_div=c["out_div"])
            h64 = r1["ref"]
            d2 = dict(x=h64.astype(np.float32), w=pw["w2"], bias=pw["b2"], res=xh, old=old if c["accumulate"] else None)
            r2 = kr.conv_reference(c2, d2, mode)
            # conv2 on the float64 h (not on its float32 rounding): the rounding of h is one more u |h| inside bar1
            bar1 = r1["bar"] + kr.U * np.abs(h64)
            if mode == 1:   # hi + lo follows its operand to 2^-17 (two bf16 roundings), for the kernel's h and for the reference's: 2^-16 |h|
                bar1 = bar1 + 2.0 ** -16 * np.abs(h64)
            a_bar = kr.conv_gather(dict(c2, in_slope=1.0), bar1.astype(np.float32)).astype(np.float64).reshape(B * T, KW * C)
            prop = (a_bar @ np.abs(pw["w2"].reshape(C, KW * C).astype(np.float64)).T).reshape(B, T, C) / c["out_div"]
            err = np.abs(got.astype(np.float64) - r2["ref"])
            worst = float(np.max(err / (prop + r2["bar"])))
            print(f"resblock_pair {c['name']} mode {mode}: worst err/bar against the float64 composite {worst:.3g}")
            record("resblock_pair", case=c["name"], mode=mode, elem=worst)
            assert worst <= 1.0, worst


@pytest.mark.parametrize("c", kc.CHAIN_CASES, ids=lambda c: c["name"])
def test_resblock_chain_rb_and_stage_are_compositions_of_pairs(kh, c):
    """launch_resblock_chain (modes 1, 2), launch_rb_bf16 (plain bf16) and, at 32 channels, launch_rb_bf16_stage bit for bit against the
    chain of pair compositions built from conv_gemm launches."""
    B, T, C, KW, dil = c["B"], c["T"], c["C"], c["KW"], c["dil"]
    assert kh.resblock_chain_supported(C, KW, dil)
    r = kr.rng_of(c["name"])
    xh = r.standard_normal((B, T, C), np.float32)
    old = r.standard_normal((B, T, C), np.float32)
    pws = _pair_weights(c["name"] + "_w", C, KW, 3)
    ws = [w for p in pws for w in (p["w1"], p["w2"])]
    for mode in (1, 2):
        x = Guarded(xh)
        flat, frag, per, bimg = _images(kh, ws, mode, C, KW)
        b1, b2 = [Guarded(p["b1"]) for p in pws], [Guarded(p["b2"]) for p in pws]
        mk = lambda: Guarded(old) if c["accumulate"] else Guarded(shape=(B, T, C), sentinel=SENTINEL)   # noqa: E731
        cur, bufs = x, []
        for m in range(3):
            last = m == 2
            nxt = mk() if last else Guarded(shape=(B, T, C), sentinel=SENTINEL)
            _compose_pair(kh, cur.ptr, nxt.ptr, flat[2 * m], flat[2 * m + 1], b1[m], b2[m], B, T, C, KW, dil[m], mode, 0.1, c["accumulate"] and last,
                          c["out_div"] if last else 1.0, frag.ptr + 4 * per * 2 * m, frag.ptr + 4 * per * (2 * m + 1))
            bufs.append(nxt)
            cur = nxt
        want, ok = cur.fetch()
        assert ok and np.all(np.isfinite(want))
        out = mk()
        msg = kh.resblock_chain(x.ptr, frag.ptr, [b.ptr for b in b1], [b.ptr for b in b2], out.ptr, B, T, C, dil, T * C, T * C, KW=KW, slope=0.1,
                                accumulate=int(c["accumulate"]), out_div=c["out_div"], mode=mode)
        assert msg is None, msg
        got, ok = out.fetch()
        assert ok and x.unchanged()
        assert np.all(bits_equal(got, want)), f"resblock_chain mode {mode} differs from its pairs: kernels.h promises the same bits"
        if mode != 2:
            continue
        member = dict(x=x.ptr, bimg=[(bimg[2 * m].ptr, bimg[2 * m + 1].ptr) for m in range(3)], b1=[b.ptr for b in b1], b2=[b.ptr for b in b2], dil=dil,
                      KW=KW, accumulate=int(c["accumulate"]), out_div=c["out_div"])
        rb = mk()
        assert kh.rb_bf16_supported([dict(member, out=rb.ptr)], 3, B, T, C, T * C, T * C)
        assert kh.rb_bf16_group([dict(member, out=rb.ptr)], 3, B, T, C, T * C, T * C) is None
        grb, ok = rb.fetch()
        assert ok and np.all(bits_equal(grb, want)), "rb_bf16 differs from the pair launches in mode 2: kernels.h promises the same bits"
        if C == 32 and not c["accumulate"]:
            # a stage of three members on the same input (here the same ResBlock three times over with different dilation orders):
            # out = ((rb_0 + rb_1) + rb_2) / 3 against three rb_bf16 launches that accumulate into one buffer
            dils = [dil, dil[::-1], [dil[1], dil[0], dil[2]]]
            acc = Guarded(shape=(B, T, C), sentinel=SENTINEL)
            for i, dd in enumerate(dils):
                mem = dict(member, out=acc.ptr, dil=dd, accumulate=int(i > 0), out_div=3.0 if i == 2 else 1.0)
                assert kh.rb_bf16_group([mem], 3, B, T, C, T * C, T * C) is None
            wants, ok = acc.fetch()
            st = Guarded(shape=(B, T, C), sentinel=SENTINEL)
            mems = [dict(member, out=st.ptr, dil=dd, accumulate=0, out_div=1.0) for dd in dils]
            assert kh.rb_bf16_supported(mems, 3, B, T, C, T * C, T * C, stage=True)
            assert kh.rb_bf16_group(mems, 3, B, T, C, T * C, T * C, stage=True) is None
            gst, ok2 = st.fetch()
            assert ok and ok2 and np.all(np.isfinite(gst))
            assert np.all(bits_equal(gst, wants)), "rb_bf16_stage differs from the accumulated rb_bf16 launches: kernels.h promises the same bits"


def _to16(x, fp16):
    """float32 -> the 16-bit patterns of its fp16 / bf16 rounding (nearest even)."""
    if fp16:
        return np.ascontiguousarray(x.astype(np.float16)).view(np.uint16)
    return (np.ascontiguousarray(kr.bf16_round(x)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def _from16(u, fp16):
    return u.view(np.float16).astype(np.float32) if fp16 else (u.astype(np.uint32) << np.uint32(16)).view(np.float32)


SENT16 = np.uint16(0xC640)   # -12288 in bf16, -6.25 in fp16


@pytest.mark.parametrize("act16", [1, 2], ids=["bf16_act", "fp16_act"])
@pytest.mark.parametrize("c", kc.CHAIN_CASES, ids=lambda c: c["name"])
def test_act16_pair_chain_and_stage_forms_agree(kh, c, act16):
    """16-bit activations (tests/act16_ref.py restates their rounding points): launch_pair_bf16 in mode 3 / 4 three times over against
    launch_rb_bf16 with act16 = 1 / 2, and at 32 channels launch_rb_bf16_stage against accumulated launch_rb_bf16 launches: bit for bit."""
    B, T, C, KW, dil = c["B"], c["T"], c["C"], c["KW"], c["dil"]
    fp16 = act16 == 2
    r = kr.rng_of(c["name"] + "_16")
    x = Guarded(_to16(r.standard_normal((B, T, C), np.float32), fp16))
    old16 = _to16(r.standard_normal((B, T, C), np.float32), fp16)
    pws = _pair_weights(c["name"] + "_w", C, KW, 3)
    imgs, keep = [], []
    for p in pws:
        for w in (p["w1"], p["w2"]):
            src = Guarded(w if fp16 else kr.pack_x3(w))
            g = Guarded(shape=(kh.bf16_image_bytes(C, KW, C) // 4,), sentinel=SENTINEL)
            assert (kh.f16_image if fp16 else kh.bf16_image)(src.ptr, g.ptr, C, KW, C) is None
            assert g.fetch()[1]
            imgs.append(g)
            keep.append(src)
    b1, b2 = [Guarded(p["b1"]) for p in pws], [Guarded(p["b2"]) for p in pws]
    mk = lambda: Guarded(old16) if c["accumulate"] else Guarded(shape=(B, T, C), dtype=np.uint16, sentinel=SENT16)   # noqa: E731
    cur = x
    for m in range(3):
        last = m == 2
        nxt = mk() if last else Guarded(shape=(B, T, C), dtype=np.uint16, sentinel=SENT16)
        pa = dict(x=cur.ptr, out=nxt.ptr, b1=b1[m].ptr, b2=b2[m].ptr, B=B, T=T, C=C, KW=KW, dil=dil[m], x_bs=T * C, out_bs=T * C, slope=0.1,
                  accumulate=int(c["accumulate"] and last), out_div=c["out_div"] if last else 1.0, mode=2 + act16, bimg1=imgs[2 * m].ptr, bimg2=imgs[2 * m + 1].ptr)
        assert kh.pair_bf16_supported(**pa)
        assert kh.pair_bf16(**pa) is None
        cur = nxt
    want, ok = cur.fetch()
    assert ok and x.unchanged() and np.all(np.isfinite(_from16(want, fp16)))
    member = dict(x=x.ptr, bimg=[(imgs[2 * m].ptr, imgs[2 * m + 1].ptr) for m in range(3)], b1=[b.ptr for b in b1], b2=[b.ptr for b in b2], dil=dil, KW=KW,
                  accumulate=int(c["accumulate"]), out_div=c["out_div"])
    rb = mk()
    assert kh.rb_bf16_supported([dict(member, out=rb.ptr)], 3, B, T, C, T * C, T * C, act16=act16)
    assert kh.rb_bf16_group([dict(member, out=rb.ptr)], 3, B, T, C, T * C, T * C, act16=act16) is None
    got, ok = rb.fetch()
    assert ok and np.array_equal(got, want), "rb_bf16 with 16-bit activations differs from three pair_bf16 launches"
    if C == 32 and not c["accumulate"]:
        dils = [dil, dil[::-1], [dil[1], dil[0], dil[2]]]
        acc = Guarded(shape=(B, T, C), dtype=np.uint16, sentinel=SENT16)
        for i, dd in enumerate(dils):
            mem = dict(member, out=acc.ptr, dil=dd, accumulate=int(i > 0), out_div=3.0 if i == 2 else 1.0)
            assert kh.rb_bf16_group([mem], 3, B, T, C, T * C, T * C, act16=act16) is None
        wants, ok = acc.fetch()
        st = Guarded(shape=(B, T, C), dtype=np.uint16, sentinel=SENT16)
        mems = [dict(member, out=st.ptr, dil=dd, accumulate=0, out_div=1.0) for dd in dils]
        assert kh.rb_bf16_supported(mems, 3, B, T, C, T * C, T * C, act16=act16, stage=True)
        assert kh.rb_bf16_group(mems, 3, B, T, C, T * C, T * C, act16=act16, stage=True) is None
        gst, ok2 = st.fetch()
        assert ok and ok2 and np.array_equal(gst, wants), "rb_bf16_stage with 16-bit activations differs from the accumulated rb_bf16 launches"


# ---------------------------------------------------------------- 16-bit activations, per element (kernel_ref's last section)
KINDS = [kr.A16_BF16, kr.A16_FP16]
KIND_IDS = ["bf16_act", "fp16_act"]


def _g16(x, kind):
    return Guarded(kr.bits16(x, kind))


def _out16(shape, old=None, kind=None):
    return _g16(old, kind) if old is not None else Guarded(shape=shape, dtype=np.uint16, sentinel=SENT16)


def _wimage(kh, w, kind, tap_split=0):
    """(source buffer, image buffer as uint16) of weights [Cout, KW, Cin]: launch_f16_image from the fp32 weights for fp16, else
    launch_bf16_image from the split-precision image (kind 0 = mode 2 and bf16 activations share it)."""
    Cout, KW, Cin = w.shape
    fp16 = kind == kr.A16_FP16
    src = Guarded(w.reshape(Cout, KW * Cin) if fp16 else kr.pack_x3(w))
    img = Guarded(shape=(kh.bf16_image_bytes(Cout, KW, Cin, tap_split) // 2,), dtype=np.uint16, sentinel=SENT16)
    msg = (kh.f16_image if fp16 else kh.bf16_image)(src.ptr, img.ptr, Cout, KW, Cin, tap_split)
    assert msg is None, msg
    bits, ok = img.fetch()
    assert ok and src.unchanged(), "the image maker wrote outside its buffer or changed its input"
    img.host = img.dev.cpu().numpy().copy()          # an input from here on
    return src, img, bits.reshape(-1)


class A16Rig:
    """Device buffers of one 16-bit-activation launch of conv_bf16 (a case of kernel_cases.A16_CASES, data of kernel_ref.a16_data)."""

    def __init__(self, kh, c, kind, d):
        self.kh, self.c, self.kind, self.d = kh, c, kind, d
        self.x = _g16(d["x"], kind) if c["in16"] else Guarded(d["x"])
        self.adds = [_g16(a, kind) for a in d["adds"]]
        self.src, self.img, self.img_bits = _wimage(kh, d["w"], kind, c["zts"])
        self.bias = Guarded(d["bias"]) if d["bias"] is not None else None
        self.res = _g16(d["res"], kind) if d["res"] is not None else None

    def args(self, out):
        c = self.c
        ad = [a.ptr for a in self.adds] + [None] * 3
        return dict(**{"in": self.x.ptr}, in_bf16=int(c["in16"]), in_slope=c["in_slope"], in_add0=ad[0], in_add1=ad[1], in_add2=ad[2], in_div=c["in_div"],
                    wimg=self.img.ptr, KWe=2 if c["zts"] else c["KW"], tap_split=c["zts"], bias=self.bias.ptr if self.bias else None,
                    act_slope=c["act_slope"], res=self.res.ptr if self.res else None, accumulate=int(c["accumulate"]), out_div=c["out_div"], out_b=out.ptr,
                    B=c["B"], T=c["T"], Cin=c["Cin"], Cout=c["Cout"], KW=c["KW"], dil=c["dil"], pad=c["pad"], rows_hint=c["rows_hint"], act16=self.kind)

    def inputs_unchanged(self):
        return all(g is None or g.unchanged() for g in [self.x, self.src, self.img, self.bias, self.res] + self.adds)

    def run(self):
        """Launch; the output as float32 holding 16-bit values.  Bands intact, inputs unchanged."""
        c = self.c
        out = _out16((c["B"], c["T"], c["Cout"]), self.d["old"], self.kind)
        assert self.kh.conv_bf16_class(**self.args(out)) == c["reach"]["bcls"]
        msg = self.kh.conv_bf16(**self.args(out))
        assert msg is None, (c["name"], msg)
        got, ok = out.fetch()
        assert ok, f"{c['name']}: wrote outside the output (guard band changed)"
        assert self.inputs_unchanged(), f"{c['name']}: an input buffer changed"
        return kr.from_bits16(got, self.kind)


def _describe_mismatch(got, want, kind):
    bad = np.argwhere(kr.bits16(got, kind) != kr.bits16(want, kind))
    first = [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in bad[:6]]
    return f"{len(bad)} of {got.size} elements differ; rows {sorted({int(i[1]) for i in bad})[:12]}, columns {sorted({int(i[2]) for i in bad})[:12]}; (index, got, want) {first}"


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("c", kc.A16_CASES, ids=lambda c: c["name"])
def test_conv_bf16_act16_exact_and_general(kh, c, kind):
    """launch_conv_bf16 with 16-bit activations.  Exact tier: on grid data whose sums are exact in float32 in any order, every output
    element equals the restatement bit for bit.  General tier (launches of at least AGG_MIN_ELEMS elements): zero-mean Gaussian data under the
    interval rule at the case's own size; Gaussian data about a cancelling mean, in a launch large enough to count flips, under the interval
    rule on every element and the aggregate rule on the share of flipped elements."""
    d = kr.a16_data(c, kind)
    want = kr.a16_exact(c, kind, d)
    got = A16Rig(kh, c, kind, d).run()
    same = kr.bits16(got, kind) == kr.bits16(want, kind)
    print(f"conv_bf16 act16 {c['name']} {kr.A16_NAME[kind]}: exact tier {int(np.sum(~same))} of {same.size} elements differ")
    record("act16_exact", case=c["name"], kind=kind, differ=int(np.sum(~same)), elems=int(same.size))
    assert np.all(same), (c["name"], kr.A16_NAME[kind], _describe_mismatch(got, want, kind))
    if same.size < kr.AGG_MIN_ELEMS:
        return
    z = kr.a16_data(c, kind, "zero_mean")          # plain Gaussian data at the case's own size: the interval rule alone
    outside, one_value = kr.check_a16_interval(c, kind, z, A16Rig(kh, c, kind, z).run())
    print(f"conv_bf16 act16 {c['name']} {kr.A16_NAME[kind]}: zero-mean data: {outside} of {same.size} outside their interval, one-value intervals {one_value:.3g}")
    record("act16_zero_mean", case=c["name"], kind=kind, outside=outside, one_value=one_value, elems=int(same.size))
    assert outside == 0, (c["name"], kr.A16_NAME[kind], outside)
    cg = kr.a16_general_case(c)
    g = kr.a16_data(cg, kind, "general")
    gg = A16Rig(kh, cg, kind, g).run()
    r = kr.check_a16_general(cg, kind, g, gg)
    print(f"conv_bf16 act16 {c['name']} {kr.A16_NAME[kind]}: general tier over {gg.size} elements: {r['outside']} outside their interval, flip share "
          f"{r['share']:.3g} (yardstick {r['yard']:.3g}), one-value intervals {r['one_value']:.3g}")
    record("act16_general", case=c["name"], kind=kind, outside=r["outside"], share=r["share"], yard=r["yard"], one_value=r["one_value"], elems=int(gg.size))
    assert r["ok"], (c["name"], kr.A16_NAME[kind], r["why"])


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", ["a_128x32_t1", "a_128x32_t31", "a_128x32_t33_pre", "a_32x128_poly", "a_64x128_t64"])
def test_weight_images_hold_the_rounded_weights_in_the_documented_order(kh, name, kind):
    """launch_bf16_image / launch_f16_image: the image decoded on the host is the weights rounded once, in kernels.h's order (Cin 8, 40 and 80:
    the zeroed channel tail; the polyphase image's two live taps per tile)."""
    c = kc.A16_BY_NAME[name]
    w = kr.a16_data(c, kind, "general")["w"]
    _, _, bits = _wimage(kh, w, kind, c["zts"])
    want = kr.a16_image_reference(w, kind, c["zts"]).reshape(-1)
    assert bits.shape == want.shape
    bad = np.flatnonzero(bits != want)
    assert bad.size == 0, f"{bad.size} image elements differ, first at {bad[:8]}"


def _bconv2(kh, c, img, **a):
    act_slope = {kc.ACT_NONE: 1.0, kc.ACT_RELU: 0.0, kc.ACT_LRELU: c["act_slope"]}[c["act"]]
    base = dict(wimg=img.ptr, KWe=2 if c["zts"] else c["KW"], tap_split=c["zts"], act_slope=act_slope, accumulate=int(c["accumulate"]), out_div=c["out_div"],
                B=c["B"], T=c["T"], Cin=c["Cin"], Cout=c["Cout"], KW=c["KW"], dil=c["dil"], pad=c["pad"], in_slope=c["in_slope"])
    return kh.conv_bf16(**{**base, **a})


def test_conv_bf16_mode2_handovers(kh):
    """Mode 2's options that no other kernel-level test launches, each against a launch that test_conv_bf16 holds to float64: a bf16 input
    (in_bf16) gives the bits of the fp32 launch on the same bf16 values; in_add / in_div gives the bits of a launch on the input summed
    beforehand in numpy float32 (the polyphase case); out_b is bf16(max(v, v * outb_slope)) of the same launch's fp32 out."""
    by = {c["name"]: c for c in kc.BCONV_CASES}
    # ---- in_bf16 (taken as it is: no input activation)
    c = dict(by["b_64x64"], in_slope=1.0)
    d = kr.conv_data(c)
    x16 = kr.bf16_round(d["x"])
    _, img, _ = _wimage(kh, d["w"], 0)
    bias, res = Guarded(d["bias"]), Guarded(d["res"])
    xa, xb = Guarded(x16), _g16(x16, kr.A16_BF16)
    outs = []
    for x, flag in ((xa, 0), (xb, 1)):
        o = Guarded(shape=(c["B"], c["T"], c["Cout"]), sentinel=SENTINEL)
        assert _bconv2(kh, c, img, **{"in": x.ptr}, in_bf16=flag, bias=bias.ptr, res=res.ptr, out=o.ptr) is None
        got, ok = o.fetch()
        assert ok and x.unchanged() and np.all(np.isfinite(got))
        outs.append(got)
    assert np.all(bits_equal(outs[0], outs[1])), "a bf16 input does not give the bits of the fp32 launch on the same values"
    # ---- in_add / in_div on the polyphase case
    c = by["b_poly"]
    d = kr.conv_data(c)
    r = kr.rng_of("b_poly_adds")
    addh = [r.standard_normal(d["x"].shape, np.float32) for _ in range(3)]
    _, img, _ = _wimage(kh, d["w"], 0, c["zts"])
    bias = Guarded(d["bias"])
    for n_add, div in ((1, 1.0), (2, 3.0), (3, 3.0)):
        pre = d["x"]
        for a in addh[:n_add]:
            pre = (pre + a).astype(np.float32)
        if div != 1.0:
            pre = (pre / np.float32(div)).astype(np.float32)
        x, xs, adds = Guarded(d["x"]), Guarded(pre), [Guarded(a) for a in addh[:n_add]]
        ad = [a.ptr for a in adds] + [None] * 3
        o1, o2 = (Guarded(shape=(c["B"], c["T"], c["Cout"]), sentinel=SENTINEL) for _ in range(2))
        assert _bconv2(kh, c, img, **{"in": x.ptr}, in_add0=ad[0], in_add1=ad[1], in_add2=ad[2], in_div=div, bias=bias.ptr, out=o1.ptr) is None
        assert _bconv2(kh, c, img, **{"in": xs.ptr}, bias=bias.ptr, out=o2.ptr) is None
        (g1, ok1), (g2, ok2) = o1.fetch(), o2.fetch()
        assert ok1 and ok2 and x.unchanged() and all(a.unchanged() for a in adds) and np.all(np.isfinite(g1))
        assert np.all(bits_equal(g1, g2)), f"in_add x {n_add} / in_div {div} differs from the launch on the summed input"
    # ---- out_b beside out
    c = by["b_128x32"]
    d = kr.conv_data(c)
    _, img, _ = _wimage(kh, d["w"], 0)
    x, bias = Guarded(d["x"]), Guarded(d["bias"])
    for slope in (1.0, 0.1):
        o, ob = Guarded(shape=(c["B"], c["T"], c["Cout"]), sentinel=SENTINEL), _out16((c["B"], c["T"], c["Cout"]))
        assert _bconv2(kh, c, img, **{"in": x.ptr}, bias=bias.ptr, out=o.ptr, out_b=ob.ptr, outb_slope=slope) is None
        (g, ok1), (gb, ok2) = o.fetch(), ob.fetch()
        assert ok1 and ok2 and np.all(np.isfinite(g))
        want = kr.bits16(np.maximum(g, g * np.float32(slope)).astype(np.float32), kr.A16_BF16)
        assert np.array_equal(gb, want), "out_b is not bf16(max(v, v * outb_slope)) of the launch's own fp32 out"
        ob2 = _out16((c["B"], c["T"], c["Cout"]))      # out_b alone
        assert _bconv2(kh, c, img, **{"in": x.ptr}, bias=bias.ptr, out_b=ob2.ptr, outb_slope=slope) is None
        assert np.array_equal(ob2.fetch()[0], want)


PAIR16_CASES = kc.PAIR_CASES + [dict(kc.PAIR_CASES[0], name="pair_c32_t1", T=1), dict(kc.PAIR_CASES[1], name="pair_c64_t33", T=33),
                                dict(kc.PAIR_CASES[2], name="pair_c128_t129", T=129)]


def _pair16_setup(kh, name, B, T, C, KW, kind):
    """Gaussian 16-bit x and running sum, weights and images of one pair; kind 0: mode 2 (fp32 tensors)."""
    r = kr.rng_of(f"{name}/{kind}/{KW}")
    xh, oldh = r.standard_normal((B, T, C), np.float32), r.standard_normal((B, T, C), np.float32)
    pw = _pair_weights(f"{name}_w{KW}", C, KW, 1)[0]
    k1, k2 = _wimage(kh, pw["w1"], kind), _wimage(kh, pw["w2"], kind)
    if kind:
        xh, oldh = kr.act16_round(xh, kind), kr.act16_round(oldh, kind)
    return dict(xh=xh, oldh=oldh, x=_g16(xh, kind) if kind else Guarded(xh), b1=Guarded(pw["b1"]), b2=Guarded(pw["b2"]), i1=k1[1], i2=k2[1], keep=(k1, k2), pw=pw)


def _pair_out(s, kind, accumulate, shape):
    if kind:
        return _out16(shape, s["oldh"] if accumulate else None, kind)
    return Guarded(s["oldh"]) if accumulate else Guarded(shape=shape, sentinel=SENTINEL)


def _pair_args(s, out, B, T, C, KW, dil, kind, accumulate, out_div):
    return dict(x=s["x"].ptr, b1=s["b1"].ptr, b2=s["b2"].ptr, out=out.ptr, B=B, T=T, C=C, KW=KW, dil=dil, slope=0.1, accumulate=int(accumulate), out_div=out_div,
                mode=2 + kind, bimg1=s["i1"].ptr, bimg2=s["i2"].ptr)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("c", PAIR16_CASES, ids=lambda c: c["name"])
def test_pair_bf16_act16_is_two_conv_bf16_launches(kh, c, kind):
    """launch_pair_bf16 in mode 3 / 4 bit for bit against two launch_conv_bf16 launches with 16-bit activations -- launches of the kind
    test_conv_bf16_act16_exact_and_general pins per element: h = r(lrelu(r(c1(r(lrelu(x))) + b1))), out = r(r(c2(h) + b2) + x) (+ sum, / div).
    With test_act16_pair_chain_and_stage_forms_agree this ties rb_bf16 and rb_bf16_stage to the same reference."""
    B, T, C, KW, dil = c["B"], c["T"], c["C"], c["KW"], c["dil"]
    s = _pair16_setup(kh, c["name"], B, T, C, KW, kind)
    fused = _pair_out(s, kind, c["accumulate"], (B, T, C))
    pa = _pair_args(s, fused, B, T, C, KW, dil, kind, c["accumulate"], c["out_div"])
    assert kh.pair_bf16_supported(x_bs=T * C, out_bs=T * C, **pa)
    assert kh.pair_bf16(x_bs=T * C, out_bs=T * C, **pa) is None
    got, ok = fused.fetch()
    assert ok and s["x"].unchanged()
    h = _out16((B, T, C))
    two = _pair_out(s, kind, c["accumulate"], (B, T, C))
    common = dict(in_bf16=1, B=B, T=T, Cin=C, Cout=C, KW=KW, KWe=KW, act16=kind)
    assert kh.conv_bf16(**{"in": s["x"].ptr}, in_slope=0.1, wimg=s["i1"].ptr, bias=s["b1"].ptr, act_slope=0.1, out_b=h.ptr, dil=dil, pad=dil * (KW - 1) // 2, **common) is None
    assert kh.conv_bf16(**{"in": h.ptr}, wimg=s["i2"].ptr, bias=s["b2"].ptr, res=s["x"].ptr, accumulate=int(c["accumulate"]), out_div=c["out_div"], out_b=two.ptr,
                        dil=1, pad=(KW - 1) // 2, **common) is None
    want, ok2 = two.fetch()
    assert ok2 and h.fetch()[1] and np.all(np.isfinite(kr.from_bits16(want, kind)))
    assert np.array_equal(got, want), _describe_mismatch(kr.from_bits16(got, kind), kr.from_bits16(want, kind), kind)


GROUP_MEMBERS = [(3, 1), (7, 1), (11, 5), (3, 5)]       # (KW, dilation) of the members, longest halo not first


@pytest.mark.parametrize("kind", [0] + KINDS, ids=["bf16"] + KIND_IDS)
@pytest.mark.parametrize("n", [2, 4])
def test_conv_bf16_group_members_get_what_they_get_alone(kh, n, kind):
    """launch_conv_bf16_group in mode 2 and with 16-bit activations: members of different kernel size, dilation, weights and buffers; each
    result is the member's own launch_conv_bf16, bit for bit (the group may run another tile shape: same order of terms)."""
    B, T, Cin, Cout = 2, 129, 32, 64
    mems, outs, rigs = [], [], []
    for i, (KW, dil) in enumerate(GROUP_MEMBERS[:n]):
        c = kc._acase(f"grp{i}", "", B, T, Cin, Cout, KW, dil, in_slope=0.1, act_slope=0.1 if i % 2 else 1.0, res=True, accumulate=bool(i % 2), out_div=3.0 if i % 2 else 1.0)
        if kind:
            d = kr.a16_data(c, kind, "general")
            rig = A16Rig(kh, c, kind, d)
            mk = lambda d=d, c=c: _out16((B, T, Cout), d["old"], kind)   # noqa: E731
            base = {k: v for k, v in rig.args(mk()).items() if k != "rows_hint"}
        else:
            cd = dict(c, bias=True)
            d = kr.conv_data(cd)
            _, img, _ = _wimage(kh, d["w"], 0)
            x, bias, res = Guarded(d["x"]), Guarded(d["bias"]), Guarded(d["res"])
            rig = (x, bias, res, img)
            mk = lambda d=d, c=c: Guarded(d["old"]) if c["accumulate"] else Guarded(shape=(B, T, Cout), sentinel=SENTINEL)   # noqa: E731
            base = dict(**{"in": x.ptr}, in_slope=0.1, wimg=img.ptr, KWe=KW, bias=bias.ptr, act_slope=c["act_slope"], res=res.ptr, accumulate=int(c["accumulate"]),
                        out_div=c["out_div"], B=B, T=T, Cin=Cin, Cout=Cout, KW=KW, dil=dil, pad=c["pad"])
        alone, grouped = mk(), mk()
        key = "out_b" if kind else "out"
        assert kh.conv_bf16(**{**base, key: alone.ptr}) is None
        mems.append({**base, key: grouped.ptr})
        outs.append((alone, grouped))
        rigs.append(rig)
    assert kh.conv_bf16_group(mems) is None
    for i, (alone, grouped) in enumerate(outs):
        (a, ok1), (g, ok2) = alone.fetch(), grouped.fetch()
        assert ok1 and ok2
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), f"member {i} of {n} differs from its own launch"


@pytest.mark.parametrize("kind", [0] + KINDS, ids=["bf16"] + KIND_IDS)
@pytest.mark.parametrize("n", [2, 4])
def test_pair_bf16_group_members_get_what_they_get_alone(kh, n, kind):
    B, T, C = 2, 129, 32
    mems, outs, keep = [], [], []
    for i, (KW, dil) in enumerate(GROUP_MEMBERS[:n]):
        s = _pair16_setup(kh, f"pgrp{i}", B, T, C, KW, kind)
        acc, div = bool(i % 2), 3.0 if i % 2 else 1.0
        alone, grouped = (_pair_out(s, kind, acc, (B, T, C)) for _ in range(2))
        pa = _pair_args(s, alone, B, T, C, KW, dil, kind, acc, div)
        assert kh.pair_bf16(x_bs=T * C, out_bs=T * C, **pa) is None
        mems.append(dict(pa, out=grouped.ptr))
        outs.append((alone, grouped))
        keep.append(s)
    assert kh.pair_bf16_group(mems) is None
    for i, (alone, grouped) in enumerate(outs):
        (a, ok1), (g, ok2) = alone.fetch(), grouped.fetch()
        assert ok1 and ok2 and keep[i]["x"].unchanged()
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), f"member {i} of {n} differs from its own launch"


@pytest.mark.parametrize("kind", [0] + KINDS, ids=["bf16"] + KIND_IDS)
def test_rb_bf16_group_of_three_members_get_what_they_get_alone(kh, kind):
    """launch_rb_bf16_group with three members (kernel sizes 3, 7, 11; their own inputs, weights and dilations): each member's launch alone."""
    B, T, C, n_pairs = 2, 257, 32, 3
    mems, outs, keep = [], [], []
    for i, (KW, dils) in enumerate([(3, [1, 3, 5]), (7, [1, 3, 5]), (11, [5, 1, 3])]):
        ss = [_pair16_setup(kh, f"rbgrp{i}_{m}", B, T, C, KW, kind) for m in range(n_pairs)]
        acc, div = bool(i % 2), 3.0 if i % 2 else 1.0
        alone, grouped = (_pair_out(ss[0], kind, acc, (B, T, C)) for _ in range(2))
        mem = dict(x=ss[0]["x"].ptr, bimg=[(s["i1"].ptr, s["i2"].ptr) for s in ss], b1=[s["b1"].ptr for s in ss], b2=[s["b2"].ptr for s in ss], dil=dils, KW=KW,
                   accumulate=int(acc), out_div=div)
        assert kh.rb_bf16_supported([dict(mem, out=alone.ptr)], n_pairs, B, T, C, T * C, T * C, act16=kind)
        assert kh.rb_bf16_group([dict(mem, out=alone.ptr)], n_pairs, B, T, C, T * C, T * C, act16=kind) is None
        mems.append(dict(mem, out=grouped.ptr))
        outs.append((alone, grouped))
        keep.append(ss)
    assert kh.rb_bf16_group(mems, n_pairs, B, T, C, T * C, T * C, act16=kind) is None
    for i, (alone, grouped) in enumerate(outs):
        (a, ok1), (g, ok2) = alone.fetch(), grouped.fetch()
        assert ok1 and ok2 and keep[i][0]["x"].unchanged()
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), f"member {i} differs from its own launch"


def test_mixed_groups_are_refused_and_write_nothing(kh):
    """A group whose members differ in element kind or geometry returns the documented message before any launch."""
    B, T, Cin, Cout = 2, 65, 32, 64
    c = kc._acase("grp_refuse", "", B, T, Cin, Cout, 3)
    rigs = [A16Rig(kh, c, kind, kr.a16_data(c, kind, "general")) for kind in KINDS]
    outs = [_out16((B, T, Cout)) for _ in rigs]
    ms = [{k: v for k, v in r.args(o).items() if k != "rows_hint"} for r, o in zip(rigs, outs)]
    share = "the members of a group share"
    assert share in kh.conv_bf16_group(ms)                                                        # bf16 beside fp16
    assert share in kh.conv_bf16_group([ms[0], dict(ms[0], T=T - 1)])                             # another T
    assert share in kh.conv_bf16_group([ms[0], dict(ms[0], Cin=Cin - 8)])
    assert "1 .. 4 members" in kh.conv_bf16_group([ms[0]] * 5)
    assert "16-bit activations write the 16-bit output alone" in kh.conv_bf16_group([ms[0], dict(ms[0], out=outs[0].ptr)])
    ss = [_pair16_setup(kh, "pgrp_refuse", B, T, 32, 3, kind) for kind in KINDS]
    pouts = [_out16((B, T, 32)) for _ in ss]
    pm = [_pair_args(s, o, B, T, 32, 3, 1, kind, False, 1.0) for s, o, kind in zip(ss, pouts, KINDS)]
    assert share in kh.pair_bf16_group(pm) and share in kh.pair_bf16_group([pm[0], dict(pm[0], T=T - 1)])
    for o in outs + pouts:
        got, ok = o.fetch()
        assert ok and np.all(got == SENT16), "a refused group wrote something"


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("c", kc.POST_CASES, ids=lambda c: c["name"])
def test_conv_post_act16(kh, c, kind):
    """launch_conv_post_bf16 in both element types (POST_CASES geometry, no join): wav holds 16-bit values inside the interval the rounded
    pre-tanh bounds give through tanh (widened by AGG_FACTOR x the float32 tanh's own deviation, post_reference's allowance for the device's
    tanhf); pcm is kr.pcm_of the kernel's own wav, exactly."""
    B, N, C, KW = c["B"], c["N"], c["C"], c["KW"]
    d = kr.post16_data(c, kind)
    lo, hi, dev = kr.post16_reference(c, kind, d)
    x, w, bias = _g16(d["x"], kind), Guarded(d["w"]), Guarded(d["bias"])
    wav = Guarded(shape=(1, B, N), sentinel=SENTINEL)
    pcm = Guarded(shape=(1, B, N), dtype=np.int16, sentinel=np.int16(-7777))
    msg = kh.conv_post_bf16(x.ptr, w.ptr, bias.ptr, wav.ptr, pcm.ptr, B, N, C, KW, fp16=kind == kr.A16_FP16)
    assert msg is None, msg
    (gw, ok_w), (gp, ok_p) = wav.fetch(), pcm.fetch()
    gw, gp = gw[0], gp[0]
    assert ok_w and ok_p and x.unchanged() and w.unchanged() and bias.unchanged()
    assert np.array_equal(gw, kr.act16_round(gw, kind)), "wav holds values that are no 16-bit values"
    inside = (gw >= lo) & (gw <= hi)
    print(f"conv_post_bf16 {c['name']} {kr.A16_NAME[kind]}: tanh deviation {dev:.3g}, {int(np.sum(~inside))} of {gw.size} outside, one-value intervals {np.mean(lo == hi):.3g}")
    record("conv_post_act16", case=c["name"], kind=kind, dev=dev, outside=int(np.sum(~inside)), one_value=float(np.mean(lo == hi)))
    assert np.all(inside), f"{int(np.sum(~inside))} samples outside their interval"
    assert np.array_equal(gp, kr.pcm_of(gw)), "pcm is not (int16)(int32)(wav * 32768) of the kernel's own wav"


# ---------------------------------------------------------------- refusals: nothing is launched
def test_wrappers_refuse_bad_arguments(kh):
    c = kc._case("refuse", 2, 65, 32, 64, 3, bias=True)
    rig = ConvRig(kh, c, 0)
    out = Guarded(shape=(2, 65, 64), ld=68, sentinel=SENTINEL)
    a = rig.args(out)
    bad = [
        (dict(a, **{"in": a["in"] + 4}), "16-byte aligned"),
        (dict(a, in_ld=28), "row stride < channels"),
        (dict(a, KW=9, dil=9, pad=0), "halo"),
        (dict(a, out_div=3.0), "out_div needs accumulate"),
        (dict(a, Cin=30), "multiples of 4"),
        (dict(a, zero_tap_split=32, KW=1, pad=0), "zero_tap_split"),
        (dict(a, act=kc.ACT_GELU, x3=2), "ACT_GELU"),
    ]
    for args, word in bad:
        msg = kh.conv_gemm(**args)
        assert msg is not None and word in msg, (word, msg)
    assert "null pointer" in kh.conv_ksplit(**a) and "null pointer" in kh.conv_rows(**a)        # no fragment-order weights
    af = dict(a, wfrag=a["w"], in_slope=0.1)
    assert "unsupported" in kh.conv_ksplit(**af) and "unsupported" in kh.conv_rows(**af)        # an input activation
    assert "unsupported" in kh.conv_ksplit(**dict(af, in_slope=1.0, x3=1))                      # exact fp32 only
    assert not kh.conv_bf16_supported(**{"in": a["in"]}, wimg=a["w"], KWe=3, B=2, T=65, Cin=32, Cout=48, KW=3, out=a["out"])
    assert "unsupported" in kh.conv_bf16(**{"in": a["in"]}, wimg=a["w"], KWe=3, B=2, T=65, Cin=32, Cout=48, KW=3, out=a["out"])
    q = Guarded(np.zeros((1, 8, 3 * 40), np.float32))
    o = Guarded(shape=(1, 8, 40), sentinel=SENTINEL)
    assert "head dim" in kh.attention(q.ptr, o.ptr, None, 1, 8, 40, 1, 0)                     # dk = 40
    assert "head dim" in kh.attention(q.ptr, o.ptr, None, 1, 8, 40, 1, 1)
    assert "aligned" in kh.attention(q.ptr + 4, o.ptr, None, 1, 8, 40, 1, 0)
    assert "position table" in kh.rel_attention(q.ptr, q.ptr, 7, q.ptr, q.ptr, o.ptr, 1, 8, 40, 1)   # pos_rows < N
    assert "head dim" in kh.rel_attention(q.ptr, q.ptr, 8, q.ptr, q.ptr, o.ptr, 1, 8, 40, 1)
    assert "head dim" in kh.rel_attention(q.ptr, q.ptr, 8, q.ptr, q.ptr, o.ptr, 1, 8, 40, 5, pos_x3=q.ptr)   # dk = 8 has no split form
    assert "multiple of 4" in kh.layernorm(q.ptr, o.ptr, q.ptr, q.ptr, None, 1, 8, 1028, 1e-5)
    assert "unaligned" in kh.layernorm(q.ptr + 4, o.ptr, q.ptr, q.ptr, None, 1, 8, 40, 1e-5)
    assert "unsupported" in kh.resblock_pair(x=q.ptr, wfrag=q.ptr, b1=q.ptr, b2=q.ptr, out=o.ptr, B=1, T=8, C=40, KW=3, dil=1, x_bs=320, out_bs=320)
    assert "out_div" in kh.resblock_pair(x=q.ptr, wfrag=q.ptr, b1=q.ptr, b2=q.ptr, out=o.ptr, B=1, T=8, C=32, KW=3, dil=1, x_bs=256, out_bs=256, out_div=3.0)
    assert "bad dims" in kh.conv_post(q.ptr, q.ptr, q.ptr, o.ptr, None, 1, 8, 30, 7)
    assert "front" in kh.conv_post(q.ptr, q.ptr, q.ptr, o.ptr, None, 1, 8, 32, 7, x_add=[None, q.ptr])
    assert "kernel odd" in kh.dwconv_swish(q.ptr, q.ptr, q.ptr, o.ptr, 1, 8, 40, 4)
    assert "bad arguments" in kh.glu(q.ptr, o.ptr, 8, 30)
    got, ok = out.fetch()
    assert ok and np.all(got == SENTINEL) and np.all(o.fetch()[0] == SENTINEL), "a refused launch wrote something"


def test_wall_time_is_recorded():
    record("wall", seconds=time.time() - _T0)


# ---------------------------------------------------------------- child process of test_conv_gemm_env_variants_in_a_child_process and of
# test_attention_serial_form_gives_the_split_forms_bits
if __name__ == "__main__":
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--child" and sys.argv[2] in kc.ENV_OF
    group = sys.argv[2]
    for k, v in kc.ENV_OF[group].items():
        assert os.environ.get(k) == v, f"{k} must be set before the library reads it"
    import kernel_harness
    kernel_harness.load()
    if group == "att_serial":   # test_attention_serial_form_gives_the_split_forms_bits: the outputs go to the file named last
        np.savez(sys.argv[3], **att_outputs_without_workspace(kernel_harness))
    for case in kc.CONV_CASES:
        if case["env"] == group:
            conv_case_body(kernel_harness, case)
    print(f"child {group} ok", flush=True)
