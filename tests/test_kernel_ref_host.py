"""CPU tests of the kernel-level differential tests' own machinery (tests/kernel_ref.py, tests/kernel_cases.py, the host-only entry points
of libe2etts_kernels_test.so): the bars pass a correct float32 result in either summation order and fail every mutation of it, the case
matrix reaches every conv_gemm / conv_bf16 tile class and the variants its table names, and the float64 references agree with
torch.nn.functional.conv1d in double, oracle/conv1d.c and oracle/ref_numpy.py's attention.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kernel_cases as kc   # noqa: E402
import kernel_ref as kr     # noqa: E402

CPU_MAX_ROWS = 4224   # B x T of a size-reduced twin (the float32 evaluations walk K one step at a time)


def cpu_twin(c):
    """The case itself, or -- where float64 and the sequential float32 evaluation would take too long -- a twin with fewer utterances:
    same T, channels, kernel and options, so the same tile edges, chunk tails and epilogue."""
    if c["B"] * c["T"] <= CPU_MAX_ROWS:
        return c
    B = max(1, CPU_MAX_ROWS // c["T"])
    t = dict(c, B=B)
    for k in ("lens", "act_rows"):
        if c[k] is not None:
            t[k] = c[k][:B]
    return t


@pytest.fixture(scope="module")
def kh():
    import __graft_entry__ as g
    assert g.built_harness_hash() == g.harness_hash(), "libe2etts_kernels_test.so is missing or stale: run `python __graft_entry__.py`"
    import kernel_harness
    kernel_harness.load()
    return kernel_harness


def _host_args(c, x3):
    """Arguments of the host-only predicates: pointers that are only tested for null are any non-zero address."""
    keep = (ctypes.c_int32 * c["B"])(*(c["act_rows"] or [0] * c["B"]))
    one = ctypes.addressof(keep)
    return keep, dict(**{"in": one}, w=one, out=one, wfrag=one if c["wfrag"] else None, bias=one if c["bias"] else None, res=one if c["res"] else None,
                      lens=one if c["lens"] is not None else None, act_rows=one if c["act_rows"] is not None else None,
                      act_rows_host=one if (c["act_rows"] is not None and c["host"]) else None,
                      B=c["B"], T=c["T"], Cin=c["Cin"], Cout=c["Cout"], KW=c["KW"], dil=c["dil"], pad=c["pad"],
                      in_bs=c["T"] * (c["Cin"] + c["in_pad"]), out_bs=c["T"] * (c["Cout"] + c["out_pad"]), res_bs=c["T"] * (c["Cout"] + c["res_pad"]),
                      in_ld=c["Cin"] + c["in_pad"], out_ld=c["Cout"] + c["out_pad"], res_ld=c["Cout"] + c["res_pad"], x3=x3, zero_tap_split=c["zts"],
                      in_slope=c["in_slope"], act=c["act"], act_slope=c["act_slope"], accumulate=int(c["accumulate"]), out_div=c["out_div"])


# ---------------------------------------------------------------- the library
def test_harness_library_exports_only_its_own_entry_points(kh):
    import __graft_entry__ as g
    out = subprocess.run(["nm", "-D", "--defined-only", g.KT_LIB], check=True, capture_output=True, text=True).stdout
    syms = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert syms and all(s.startswith("e2ekt_") for s in syms), [s for s in syms if not s.startswith("e2ekt_")]
    for want in ("e2ekt_conv_gemm", "e2ekt_conv_ksplit", "e2ekt_conv_rows", "e2ekt_conv_bf16", "e2ekt_attention", "e2ekt_rel_attention",
                 "e2ekt_layernorm", "e2ekt_resblock_pair", "e2ekt_resblock_chain", "e2ekt_pair_bf16", "e2ekt_rb_bf16_group", "e2ekt_rb_bf16_stage",
                 "e2ekt_conv_post", "e2ekt_dwconv_swish", "e2ekt_dwconv_glu_swish", "e2ekt_glu", "e2ekt_x3_to_frag", "e2ekt_f32_to_frag",
                 "e2ekt_bf16_image", "e2ekt_f16_image"):
        assert want in syms, want
    assert g.harness_hash() in kh.version()          # the harness's own staleness marker
    assert g.built_hash() == g.source_hash()         # the product library's marker keeps its meaning: the harness is not part of it


def test_byte_counts(kh):
    assert kh.x3_frag_bytes(33, 3, 36) == 2 * 3 * 2 * 4096
    assert kh.bf16_image_bytes(64, 3, 36, 0) == 2 * 2 * 3 * 2048 and kh.bf16_image_bytes(64, 3, 36, 32) == 2 * 2 * 2 * 2048
    nseg_bytes = kh.attention_workspace_bytes(2, 600, 128, 2)
    assert nseg_bytes > 0 and nseg_bytes % (2 * 2 * 600 * (64 + 2) * 4) == 0


# ---------------------------------------------------------------- coverage of the tile classes and variants
def test_conv_gemm_classes_cover_what_the_function_can_return(kh):
    seen = set()
    for c in kc.CONV_CASES:
        for x3 in kc.modes_of(c):
            keep, a = _host_args(c, x3)
            cls = kh.conv_gemm_class(**a)
            want, _ = kc.variant(c, x3)
            assert cls == want, (c["name"], x3, cls, want)     # the restatement in kernel_cases.variant() follows the library
            seen.add(cls)
            del keep
    assert seen == kc.ALL_CONV_CLASSES, (seen ^ kc.ALL_CONV_CLASSES)


@pytest.mark.parametrize("c", [c for c in kc.CONV_CASES if c["reach"]], ids=lambda c: c["name"])
def test_case_reaches_the_variant_it_is_there_for(kh, c):
    """What is pinned to the library and what is not.  The tile class comes from the library (conv_gemm_class through the harness), so a
    change of the few / half / many-rows thresholds or of the class of a shape fails here.  BFRAG, CPI, OCC, accumulate, the scalar epilogue,
    GELU and the tiles per workgroup are template arguments and locals of launch_conv_gemm that no host function reports: they are checked
    against kernel_cases.variant(), a restatement of conv_gemm.hip's launch_cfg / launch_cfg_impl.  A later change of THOSE choices in
    conv_gemm.hip does not fail this test; it has to be carried over to variant() by hand (the restatement cites the lines it follows)."""
    r = c["reach"]
    wg = 1 if c["env"] == "wg1" else 24
    for x3 in kc.modes_of(c):
        cls, v = kc.variant(c, x3, wg, c["env"] != "frag64")
        if "cls" in r:
            keep, a = _host_args(c, x3)
            assert kh.conv_gemm_class(**a) == r["cls"][1 if x3 else 0], (c["name"], x3)
        for key in ("bfrag", "cpi", "accumulate", "scalar", "gelu"):
            if key in r:
                assert v[key] == r[key], (c["name"], x3, key, v)
        if "occ3" in r:
            assert v["occ3"] == (r["occ3"] and x3 == 0), (c["name"], x3, v)
        if "narrow" in r:
            assert v["narrow"] == (x3 == 0)
        if "tpb" in r:
            assert v["tpb"] >= r["tpb"] and (c["act_rows"] is not None or ((c["T"] + int(v["tile"].split("x")[0]) - 1) // int(v["tile"].split("x")[0])) % v["tpb"] != 0), v


def test_every_variant_axis_is_reached():
    vs = [kc.variant(c, x3, 1 if c["env"] == "wg1" else 24, c["env"] != "frag64")[1] for c in kc.CONV_CASES for x3 in kc.modes_of(c)]
    assert {v["cpi"] for v in vs if v["bfrag"]} == {0, 2, 4}
    assert any(v["occ3"] for v in vs) and any(v["bfrag"] and v["tile"] == "128x128" and not v["occ3"] for v in vs)
    for tile in ("128x128", "64x128", "64x64", "256x64", "256x32"):
        assert any(v["tile"] == tile and not v["scalar"] for v in vs), tile
        assert any(v["tile"] == tile and v["accumulate"] for v in vs) or tile in ("64x128", "256x32"), tile
    assert any(v["scalar"] and v["gelu"] for v in vs) and any(v["gelu"] and v["bfrag"] for v in vs) and any(v["gelu"] and not v["bfrag"] and not v["scalar"] for v in vs)
    assert any(v["tpb"] > 1 for v in vs)
    # the axes of the issue's table
    have = lambda k: {c[k] for c in kc.CONV_CASES}   # noqa: E731
    assert {1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 513} <= have("T")
    assert {1, 2, 18, 32, 33, 64, 80, 96, 128, 130, 256, 384} <= have("Cout")
    assert {4, 32, 36, 80, 128, 192, 256} <= have("Cin")
    kd = {(c["KW"], c["dil"]) for c in kc.CONV_CASES}
    assert {(1, 1), (3, 1), (3, 5), (7, 1), (9, 1), (11, 5)} <= kd and any(k != 1 and d * (k - 1) == kc.MAX_HALO for k, d in kd)
    assert {c["act"] for c in kc.CONV_CASES} == {0, 1, 2, 3, 4, 5}
    assert {c["B"] for c in kc.CONV_CASES if c["host"]} >= {1, 3, 64, 70}
    pads = {("c" if c["pad"] == c["dil"] * (c["KW"] - 1) // 2 else "0" if c["pad"] == 0 else "L") for c in kc.CONV_CASES if c["KW"] > 1}
    assert pads == {"c", "0", "L"}


def test_supported_predicates_follow_their_restatement(kh):
    n_ks = n_rows = 0
    for c in kc.CONV_CASES:
        for x3 in kc.modes_of(c):
            keep, a = _host_args(c, x3)
            assert kh.conv_ksplit_supported(**a) == kc.ksplit_ok(c, x3), (c["name"], x3)
            assert kh.conv_rows_supported(**a) == kc.rows_ok(c, x3), (c["name"], x3)
            n_ks += kc.ksplit_ok(c, x3)
            n_rows += kc.rows_ok(c, x3)
    assert n_ks >= 8 and n_rows >= 24     # the matrix keeps a fair number of launches for both


def _bconv_args(c):
    one = 16
    return dict(**{"in": one}, wimg=one, KWe=2 if c["zts"] else c["KW"], tap_split=c["zts"], B=c["B"], T=c["T"], Cin=c["Cin"], Cout=c["Cout"],
                KW=c["KW"], dil=c["dil"], pad=c["pad"], out=one, in_slope=c["in_slope"])


def test_conv_bf16_classes_cover_what_the_function_can_return(kh):
    seen = set()
    for c in kc.BCONV_CASES:
        a = _bconv_args(c)
        assert kh.conv_bf16_supported(**a), c["name"]
        cls = kh.conv_bf16_class(**a)
        assert cls == c["reach"]["bcls"], (c["name"], cls)
        seen.add(cls)
    assert seen == kc.ALL_BCONV_CLASSES, seen ^ kc.ALL_BCONV_CLASSES
    assert not kh.conv_bf16_supported(**dict(_bconv_args(kc.BCONV_CASES[0]), Cout=48))
    assert not kh.conv_bf16_supported(**dict(_bconv_args(kc.BCONV_CASES[0]), Cin=36))


# ---------------------------------------------------------------- the references are the operations they claim to be
@pytest.mark.parametrize("name", ["t63_c18_k3d5", "t129_c96_halo64", "t255_c128_k3_left", "t65_c33_k9"])
def test_conv_reference_is_conv1d(name):
    import torch
    import torch.nn.functional as F
    c = dict(kc.CONV_BY_NAME[name], bias=True, res=False, lens=None, act=kc.ACT_NONE, accumulate=False, out_div=1.0, in_slope=1.0)
    d = kr.conv_data(c)
    ref = kr.conv_reference(c, d, 0)["ref"]
    halo = c["dil"] * (c["KW"] - 1)
    x = torch.from_numpy(d["x"]).double().permute(0, 2, 1)
    x = F.pad(x, (c["pad"], halo - c["pad"]))
    y = F.conv1d(x, torch.from_numpy(d["w"]).double().permute(0, 2, 1).contiguous(), torch.from_numpy(d["bias"]).double(), dilation=c["dil"])
    assert np.abs(y.permute(0, 2, 1).numpy() - ref).max() <= 1e-12 * (1 + np.abs(ref).max())
    if 2 * c["pad"] == halo:   # oracle/conv1d.c pads both sides alike
        import __graft_entry__ as g
        clib = os.path.join(ROOT, "oracle", "lib", "libref_conv1d.so")
        assert os.path.exists(clib), "oracle/lib/libref_conv1d.so is missing: run `python __graft_entry__.py`"
        lib = ctypes.CDLL(clib)
        lib.ref_conv1d_f32.restype = ctypes.c_int
        lib.ref_conv1d_f32.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7
        xc = np.ascontiguousarray(d["x"].transpose(0, 2, 1))
        wc = np.ascontiguousarray(d["w"].transpose(0, 2, 1))
        out = np.empty((c["B"], c["Cout"], c["T"]), np.float32)
        assert lib.ref_conv1d_f32(xc.ctypes.data, wc.ctypes.data, d["bias"].ctypes.data, out.ctypes.data, c["B"], c["Cin"], c["T"], c["Cout"], c["KW"],
                                  c["pad"], c["dil"]) == 0
        r = kr.check_conv(c, d, 0, out.transpose(0, 2, 1))      # a float32 evaluation in yet another order: inside both bars
        assert r["ok"], r["why"]


def test_attention_reference_is_the_oracles_attention():
    from oracle import ref_numpy as orc
    c = dict(name="pin_att", B=2, N=37, n_head=2, dk=64, lens=[37, 20])    # sqrt(64): the same temperature in float32 and float64
    r = kr.rng_of("pin_att")
    H = 128
    x = r.standard_normal((2, 37, H))
    W = [r.standard_normal((H, H)) / 8 for _ in range(3)]
    o = object.__new__(orc.AcousticOracle)
    o.dt, o.n_head = np.float64, 2
    o.sd = {"a.fc.weight": np.eye(H), "a.fc.bias": np.zeros(H), "a.layer_norm.weight": np.ones(H), "a.layer_norm.bias": np.zeros(H)}
    for nm, w in zip(("w_qs", "w_ks", "w_vs"), W):
        o.sd[f"a.{nm}.weight"], o.sd[f"a.{nm}.bias"] = w, np.zeros(H)
    pad = ~(np.arange(37)[None, :] < np.asarray(c["lens"])[:, None])
    want = o.mha("a", x, pad)
    qkv = np.concatenate([x @ w.T for w in W], -1)
    att, _ = kr.att_reference(c, dict(qkv=qkv))
    rows = ~pad          # the oracle leaves the masked query rows to the block's masked_fill
    got = orc.layer_norm(att + x, np.ones(H), np.zeros(H), 1e-5)
    assert np.abs(got - want)[rows].max() <= 1e-12


def test_layernorm_reference_is_the_oracles():
    from oracle import ref_numpy as orc
    for c in kc.LN_CASES:
        d = kr.ln_data(c)
        y, bar = kr.ln_reference(dict(c, lens=None), d)
        want = orc.layer_norm(d["x"].astype(np.float64), d["gamma"].astype(np.float64), d["beta"].astype(np.float64), np.float64(np.float32(d["eps"])))
        assert np.abs(y - want).max() <= 1e-12 * (1 + np.abs(want).max())
        y, bar = kr.ln_reference(c, d)
        assert np.all(np.abs(kr.ln_eval32(c, d).astype(np.float64) - y) <= bar), c["name"]
        bad = kr.ln_eval32(c, dict(d, eps=0.0))       # zero-variance rows: without eps the row is not finite
        assert not np.all(np.isfinite(bad))


# ---------------------------------------------------------------- a correct result passes
LINEAR_TWINS = [dict(c, act=kc.ACT_NONE, lin=True) for c in kc.CONV_CASES if c["act"] in kr.TRANSCENDENTAL]


@pytest.mark.slow
@pytest.mark.parametrize("c", kc.CONV_CASES + kc.BCONV_CASES + LINEAR_TWINS, ids=lambda c: c["name"] + ("_lin" if c.get("lin") else ""))
def test_float32_evaluations_sit_inside_both_bars(c):
    """Every case, and for the tanh / swish / GELU cases also the same launch with the activation off (what carries their aggregate bar)."""
    t = cpu_twin(c)
    d = kr.conv_data(t)
    for x3 in ((2,) if c in kc.BCONV_CASES else kc.modes_of(kc.CONV_BY_NAME[c["name"]])):
        ref = kr.conv_reference(t, d, x3)
        yard = kr.conv_yardstick(t, d, x3, ref)
        for order in ("blocked", "sequential", "matmul"):
            r = kr.check_conv(t, d, x3, kr.conv_eval32(t, d, x3, order=order), ref, yard)
            assert r["ok"], (x3, order, r["why"])


# ---------------------------------------------------------------- a wrong result fails
# the smallest K for which each mutation exists (K = 4 for those a Linear has, 12 and 36 for those that need taps / a chunk tail / a second
# column tile), and the largest K of the matrix (2816; the chunk-tail mutation at 11 x 80 = 880 and 11 x 36, the longest with Cin % 32 != 0)
MUT_SMALL_LIN = kc._case("mut_k4", 2, 65, 4, 33, bias=True, res=True, lens=[64, 33], accumulate=True, out_div=3.0)
MUT_SMALL_TAPS = kc._case("mut_k12", 2, 129, 4, 33, 3, bias=True, lens=[129, 70], accumulate=True, out_div=3.0)
MUT_LARGE = kc._case("mut_k2816", 2, 129, 256, 33, 11, bias=True, res=True, lens=[129, 70], accumulate=True, out_div=3.0)
MUT_LARGE_TAIL = kc._case("mut_k880", 2, 129, 80, 33, 11, bias=True, lens=[100, 129])
MUTATIONS = [
    ("drop_tap", (MUT_SMALL_TAPS, MUT_LARGE), (0, 1, 2)),
    ("shift_tile", (MUT_SMALL_TAPS, MUT_LARGE), (0, 1, 2)),
    ("drop_tail_chunk", (MUT_SMALL_LIN, MUT_SMALL_TAPS, MUT_LARGE_TAIL), (0, 1, 2)),
    ("drop_split", (MUT_SMALL_LIN, MUT_LARGE), (1,)),
    ("trunc_lo", (MUT_SMALL_LIN, MUT_LARGE), (1,)),
    ("stale_col", (MUT_SMALL_LIN, MUT_LARGE), (0, 1, 2)),
    ("mask_off_by_one", (MUT_SMALL_LIN, MUT_LARGE), (0, 1, 2)),
    ("div_before", (MUT_SMALL_LIN, MUT_LARGE), (0, 1, 2)),
]


@pytest.mark.parametrize("mut,cases,modes", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_every_mutation_fails_a_bar(mut, cases, modes):
    for c in cases:
        d = kr.conv_data(c)
        for x3 in modes:
            ref = kr.conv_reference(c, d, x3)
            yard = kr.conv_yardstick(c, d, x3, ref)
            assert kr.check_conv(c, d, x3, kr.conv_eval32(c, d, x3), ref, yard)["ok"]
            r = kr.check_conv(c, d, x3, kr.conv_eval32(c, d, x3, mut=mut), ref, yard)
            assert not r["ok"], (mut, c["name"], x3, r)


def test_a_dropped_lo_product_needs_the_aggregate_bar():
    """What the second bar is for: at K = 2816 the per-element bar alone lets a missing lo x hi product through."""
    c, x3 = MUT_LARGE, 1
    d = kr.conv_data(c)
    r = kr.check_conv(c, d, x3, kr.conv_eval32(c, d, x3, mut="drop_split"))
    assert r["elem_ratio"] <= 1.0 and r["agg_ratio"] > 1.0, r


# ---------------------------------------------------------------- attention
def att_twin(c):
    """The case, or for the B = 40 launches a twin of four utterances (the first, the last and two between: same N, heads, lengths)."""
    if c["B"] <= 3:
        return c
    pick = [0, c["B"] // 3, 2 * c["B"] // 3, c["B"] - 1]
    return dict(c, B=4, lens=[c["lens"][i] for i in pick] if c["lens"] is not None else None)


ATT_CPU = [att_twin(c) for c in kc.ATT_CASES]


@pytest.mark.parametrize("c", ATT_CPU, ids=lambda c: c["name"])
def test_attention_float32_evaluations_sit_inside_the_bar(c):
    d = kr.att_data(c)
    ref = kr.att_reference(c, d)
    for x3 in (0, 1):
        o, W, dev = kr.att_bar(c, d, x3, ref)
        assert dev < (2e-5 if x3 else 2e-6), dev        # the yardstick itself is a float32 (split-precision) evaluation, not something looser
        for seg in (None, 64):
            ok, worst = kr.check_att(kr.att_eval32(c, d, x3, seg=seg), o, W, dev)
            assert ok, (x3, seg, worst)
    assert np.all(ref[0][~(np.arange(c["N"])[None, :] < np.asarray(c["lens"] or [c["N"]] * c["B"])[:, None])] == 0)


@pytest.mark.parametrize("name", ["n65_dk32", "n600_dk64_ws"])
def test_attention_mutations_fail_the_bar(name):
    c = next(a for a in kc.ATT_CASES if a["name"] == name)
    d = kr.att_data(c)
    for x3 in (0, 1):
        o, W, dev = kr.att_bar(c, d, x3)
        ok, worst = kr.check_att(kr.att_eval32(c, d, x3, seg=32, drop_segment=True), o, W, dev)     # a softmax missing one key segment
        assert not ok, (x3, worst)
        off = dict(c, lens=[min(c["N"], n + 1) if 0 < n < c["N"] else n for n in c["lens"]])         # the key mask off by one at lens[b]
        got = kr.att_eval32(off, d, x3, seg=32)
        rows = np.arange(c["N"])[None, :] < np.asarray(c["lens"])[:, None]
        ok, worst = kr.check_att(got, o, W, dev, rows)
        assert not ok, (x3, worst)


@pytest.mark.parametrize("c", kc.REL_CASES, ids=lambda c: c["name"])
def test_rel_attention_reference(c):
    """The float32 evaluations sit inside their own bar by construction; what is pinned here is the shift: against the pad-and-reshape form of
    _relative_shift (a column of zeros in front, viewed as [N + 1, N], first row dropped) that kernels.h's index form restates."""
    d = kr.rel_data(dict(c, pos_rows=c["N"]))
    cc = dict(c, pos_rows=c["N"])
    B, N, nh, dk = c["B"], c["N"], c["n_head"], c["dk"]
    q, k, _ = kr._heads(cc, d["qkv"], np.float32)
    qv = (q + d["v"].reshape(1, nh, 1, dk)).astype(np.float32).astype(np.float64)
    qu = (q + d["u"].reshape(1, nh, 1, dk)).astype(np.float32).astype(np.float64)
    ps = qv @ d["pos"].astype(np.float64).transpose(0, 2, 1)[None]                 # [B, nh, N, N]
    padded = np.concatenate([np.zeros((B, nh, N, 1)), ps], -1).reshape(B, nh, N + 1, N)[:, :, 1:]
    want = (qu @ k.astype(np.float64).transpose(0, 1, 3, 2) + padded) / np.float64(np.float32(np.sqrt(np.float32(nh * dk))))
    got = kr.rel_scores(cc, d, np.float64)
    assert np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max())
    o, W, dev = kr.rel_bar(cc, d, False)
    assert dev < 2e-6
    ok, worst = kr.check_att(kr.rel_eval32(cc, d, False), o, W, dev)
    assert ok
    if N > 2:   # mutations: the (i, i + 1) entry taken from the table instead of 0; the lower triangle read one position row off
        for mut in ("diag", "row"):
            ok, worst = kr.check_att(kr.rel_eval32(cc, d, False, mut=mut), o, W, dev)
            assert not ok, (mut, worst)
    if c["dk"] in kc.REL_X3_DK:
        o, W, dev3 = kr.rel_bar(cc, d, True)
        assert dev <= dev3 < 3e-5, dev3              # the split-precision yardstick: above the fp32 one, below plain bf16's 2^-9
        if N > 2:
            ok, worst = kr.check_att(kr.rel_eval32(cc, d, True, mut="row"), o, W, dev3)
            assert not ok, worst


# ---------------------------------------------------------------- small kernels
@pytest.mark.parametrize("c", kc.POST_CASES, ids=lambda c: c["name"])
def test_conv_post_inputs_keep_the_boundary_share_small(c):
    wav, bar, dev = kr.post_reference(c, kr.post_data(c))
    assert 0.3 < np.abs(wav).max() < 0.999                  # the full-scale inputs: the wav bars and the conversion of the kernel's own wav
    d = kr.post_data(c, small=True)
    wav, bar, dev = kr.post_reference(c, d)
    near = kr.pcm_boundary(wav, bar)
    assert near.mean() <= 1e-3, near.mean()           # the project's PCM share: at most 0.1 % of samples may be excluded
    ref_pcm = kr.pcm_of(wav.astype(np.float32))
    assert np.abs(ref_pcm.astype(np.int32) - np.trunc(wav * 32768).astype(np.int32)).max() <= 1


def test_small_kernel_references():
    for c in kc.DW_CASES:
        d = kr.dw_data(c)
        ref, bar, dev = kr.dw_reference(c, d["x"], d["w"], d["bias"])
        x = d["x"]
        half = (c["k"] - 1) // 2
        acc = np.zeros_like(x)
        for j in range(c["k"]):       # float32, in tap order
            lo, hi = max(0, half - j), min(c["N"], c["N"] + half - j)
            if hi > lo:
                acc[:, lo:hi] += x[:, lo + j - half:hi + j - half] * d["w"][j]
        got = kr.act32(acc + d["bias"], kc.ACT_SWISH, 0.0)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= bar), c["name"]
        assert not np.all(np.abs(np.roll(got, 1, axis=1).astype(np.float64) - ref) <= bar)
    for c in kc.GLU_CASES:
        x = kr.rng_of(c["name"]).standard_normal((c["rows"], 2 * c["C"]), np.float32) * 3
        ref, bar, dev = kr.glu_reference(x)
        assert np.all(np.abs(kr.glu32(x).astype(np.float64) - ref) <= bar) and dev < 1e-6


# ---------------------------------------------------------------- fused ResBlocks and refusals through the host-only paths of the harness
def test_fused_resblock_predicates_through_the_harness(kh):
    """The *_supported entry points of the pair / chain / rb wrappers: exercises the binding's pointer-array marshalling (RB_MAX_PAIRS
    indexing, per-member arrays) without a GPU; pointers are only tested for null."""
    one = 4096
    for c in kc.PAIR_CASES:
        assert kh.resblock_pair_supported(c["C"], c["KW"], c["dil"])
        pa = dict(x=one, wfrag=one, b1=one, b2=one, out=one, B=c["B"], T=c["T"], C=c["C"], KW=c["KW"], dil=c["dil"], x_bs=c["T"] * c["C"],
                  out_bs=c["T"] * c["C"], mode=2, bimg1=one, bimg2=one)
        assert kh.pair_bf16_supported(**pa)
        assert not kh.pair_bf16_supported(**dict(pa, bimg2=None)) and not kh.pair_bf16_supported(**dict(pa, mode=1))
        assert not kh.pair_bf16_supported(**dict(pa, x_bs=c["T"] * c["C"] + 4)) and not kh.pair_bf16_supported(**dict(pa, act_rows=one))
    assert not kh.resblock_pair_supported(40, 3, 1) and not kh.resblock_pair_supported(64, 4, 1) and not kh.resblock_pair_supported(64, 11, 7)
    for c in kc.CHAIN_CASES:
        B, T, C = c["B"], c["T"], c["C"]
        assert kh.resblock_chain_supported(C, c["KW"], c["dil"])
        mem = dict(x=one, out=one, bimg=[(one, one)] * 3, b1=[one] * 3, b2=[one] * 3, dil=c["dil"], KW=c["KW"])
        assert kh.rb_bf16_supported([mem], 3, B, T, C, T * C, T * C)
        assert kh.rb_bf16_supported([mem, dict(mem, KW=7), dict(mem, dil=c["dil"][::-1])], 3, B, T, C, T * C, T * C)
        hole = dict(mem, bimg=[(one, one), (one, None), (one, one)])                       # pair 1 lacks its conv2 image
        assert not kh.rb_bf16_supported([mem, hole], 3, B, T, C, T * C, T * C)
        assert not kh.rb_bf16_supported([dict(mem, b2=[one, one, None])], 3, B, T, C, T * C, T * C)
        assert not kh.rb_bf16_supported([dict(mem, dil=[1, 3, 300])], 3, B, T, C, T * C, T * C)     # more than half a tile recomputed
        assert kh.rb_bf16_supported([mem] * 3, 3, B, T, C, T * C, T * C, stage=True) == (C == 32)
        assert not kh.rb_bf16_supported([mem, dict(mem, x=2 * one)], 3, B, T, C, T * C, T * C, stage=True)   # a stage shares its input
        assert not kh.rb_bf16_supported([mem, dict(mem, accumulate=1)], 3, B, T, C, T * C, T * C, stage=True)
    assert not kh.resblock_chain_supported(32, 5, [1, 3, 5]) and not kh.resblock_chain_supported(32, 3, [1, 3, 9]) and not kh.resblock_chain_supported(128, 3, [1, 3, 5])


def test_wrappers_refuse_bad_arguments_before_any_launch(kh):
    """Every wrapper validates on the host and returns its message instead of launching: these calls never reach the GPU runtime (the
    addresses are made up), so they run here; tests/test_gpu_kernels.py repeats them on real buffers and checks that nothing was written."""
    one = 4096
    a = dict(**{"in": one}, w=one, out=one, bias=one, B=2, T=65, Cin=32, Cout=64, KW=3, dil=1, pad=1, in_bs=65 * 36, out_bs=65 * 68, in_ld=36, out_ld=68)
    for args, word in [(dict(a, **{"in": one + 4}), "16-byte aligned"), (dict(a, in_ld=28), "row stride < channels"), (dict(a, KW=9, dil=9, pad=0), "halo"),
                       (dict(a, out_div=3.0), "out_div needs accumulate"), (dict(a, Cin=30), "multiples of 4"),
                       (dict(a, zero_tap_split=32, KW=1, pad=0), "zero_tap_split"), (dict(a, act=kc.ACT_GELU, x3=2), "ACT_GELU"),
                       (dict(a, pad=3), "pad out of range"), (dict(a, x3=3), "x3 must be"), (dict(a, in_slope=1.5), "in_slope")]:
        msg = kh.conv_gemm(**args)
        assert msg is not None and word in msg, (word, msg)
    assert "null pointer" in kh.conv_ksplit(**a) and "null pointer" in kh.conv_rows(**a)
    af = dict(a, wfrag=one, in_slope=0.1)
    assert "unsupported" in kh.conv_ksplit(**af) and "unsupported" in kh.conv_rows(**af)
    assert "unsupported" in kh.conv_ksplit(**dict(af, in_slope=1.0, x3=1))
    assert "unsupported" in kh.conv_rows(**dict(af, in_slope=1.0, KW=9, dil=3, pad=12))          # halo 24 > 16
    assert "unsupported" in kh.conv_bf16(**{"in": one}, wimg=one, KWe=3, B=2, T=65, Cin=32, Cout=48, KW=3, out=one)
    assert "head dim" in kh.attention(one, one, None, 1, 8, 40, 1, 0) and "head dim" in kh.attention(one, one, None, 1, 8, 40, 1, 1)
    assert "aligned" in kh.attention(one + 4, one, None, 1, 8, 64, 1, 0) and "bad dims" in kh.attention(one, one, None, 1, 8, 65, 2, 0)
    assert "position table" in kh.rel_attention(one, one, 7, one, one, one, 1, 8, 40, 1)
    assert "head dim" in kh.rel_attention(one, one, 8, one, one, one, 1, 8, 40, 1)
    assert "head dim" in kh.rel_attention(one, one, 8, one, one, one, 1, 8, 40, 5, pos_x3=one)
    assert "multiple of 4" in kh.layernorm(one, one, one, one, None, 1, 8, 1028, 1e-5) and "unaligned" in kh.layernorm(one + 4, one, one, one, None, 1, 8, 40, 1e-5)
    pr = dict(x=one, wfrag=one, b1=one, b2=one, out=2 * one, B=1, T=8, KW=3, dil=1, x_bs=256, out_bs=256)
    assert "unsupported" in kh.resblock_pair(C=40, **pr) and "out_div" in kh.resblock_pair(C=32, out_div=3.0, **pr)
    assert "in-place" in kh.resblock_pair(C=32, **dict(pr, out=one)) and "mode" in kh.resblock_pair(C=32, mode=3, **pr)
    assert "bad dims" in kh.conv_post(one, one, one, one, None, 1, 8, 30, 7) and "front" in kh.conv_post(one, one, one, one, None, 1, 8, 32, 7, x_add=[None, one])
    assert "kernel odd" in kh.dwconv_swish(one, one, one, 2 * one, 1, 8, 40, 4) and "bad arguments" in kh.glu(one, one, 8, 30)
