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
    assert g.built_harness_act16_hash() == g.harness_act16_hash(), "libe2etts_kernels_test.so is missing or stale: run `python __graft_entry__.py`"
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
                 "e2ekt_bf16_image", "e2ekt_f16_image", "e2ekt_conv_post_bf16", "e2ekt_conv_bf16_group", "e2ekt_pair_bf16_group"):
        assert want in syms, want
    assert g.harness_hash() in kh.version()          # the harness's own staleness marker
    assert g.harness_act16_hash() in kh.load().e2ekt_act16_version().decode()      # ... and its second source's
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


# ---------------------------------------------------------------- 16-bit activations: the case matrix, the restatement, the two tiers
KINDS = [kr.A16_BF16, kr.A16_FP16]


def _a16_host_args(c, kind):
    one = 16
    return dict(**{"in": one}, in_bf16=int(c["in16"]), in_slope=c["in_slope"], in_add0=one if c["n_add"] > 0 else None,
                in_add1=one if c["n_add"] > 1 else None, in_add2=one if c["n_add"] > 2 else None, in_div=c["in_div"], wimg=one,
                KWe=2 if c["zts"] else c["KW"], tap_split=c["zts"], bias=one, act_slope=c["act_slope"], res=one if c["res"] else None,
                accumulate=int(c["accumulate"]), out_div=c["out_div"], out_b=one, B=c["B"], T=c["T"], Cin=c["Cin"], Cout=c["Cout"], KW=c["KW"],
                dil=c["dil"], pad=c["pad"], rows_hint=c["rows_hint"], act16=kind)


@pytest.mark.parametrize("c", kc.A16_CASES, ids=lambda c: c["name"])
def test_a16_case_is_supported_reaches_its_class_and_sums_exactly(kh, c):
    for kind in KINDS:
        a = _a16_host_args(c, kind)
        assert kh.conv_bf16_supported(**a), (c["name"], kind)
        assert kh.conv_bf16_class(**a) == c["reach"]["bcls"], (c["name"], kh.conv_bf16_class(**a))
        d = kr.a16_data(c, kind)
        ratio, unit = kr.act16_exactness(c, kind, d)
        assert ratio < kr.A16_EXACT_LIMIT, (c["name"], kind, np.log2(ratio))       # the precondition of the exact tier
        pre, want = kr.a16_sum64(c, kind, d)[0], kr.a16_exact(c, kind, d)
        if c["special"] is None:   # the data exercises what the tier is for: the 16-bit rounding changes most sums
            assert np.mean(kr.act16_round(pre.astype(np.float32), kind) != pre) > 0.5, c["name"]
        if c["special"] == "inf" and kind == kr.A16_FP16:
            assert 0.02 < np.mean(np.isinf(want)) < 0.5 and not np.any(np.isnan(want))
        if c["special"] == "sub" and kind == kr.A16_FP16:
            st = kr.act16_stage(c, kind, d["x"], d["adds"])
            assert np.all(np.abs(st) < 2.0 ** -14) and np.mean((np.abs(want) < 2.0 ** -14) & (want != 0)) > 0.9


def test_a16_matrix_covers_every_axis():
    cs = kc.A16_CASES
    assert {c["reach"]["bcls"] for c in cs} == kc.ALL_BCONV_CLASSES
    for cls in kc.ALL_BCONV_CLASSES:          # every tile shape at both input kinds, and at its row edges
        mine = [c for c in cs if c["reach"]["bcls"] == cls]
        assert {c["in16"] for c in mine} == {True, False}, cls
        bm = int(cls.split("_")[-1].split("x")[0])
        assert {bm - 1, bm, bm + 1} <= {c["T"] for c in mine}, cls
    assert {1, 31, 33} <= {c["T"] for c in cs}
    halo = {c["dil"] * (c["KW"] - 1) for c in cs}
    assert 0 in halo and kc.MAX_HALO in halo
    pads = {("c" if c["pad"] == c["dil"] * (c["KW"] - 1) // 2 else "0" if c["pad"] == 0 else "L") for c in cs if c["KW"] > 1}
    assert pads == {"c", "0", "L"}
    assert {8, 40, 80, 32, 64, 256} <= {c["Cin"] for c in cs} and {32, 96, 64, 128, 256} <= {c["Cout"] for c in cs}
    assert any(not c["in16"] and c["Cin"] == 80 and c["KW"] == 7 for c in cs)                     # conv_pre taking the mel
    assert any(c["zts"] == 64 and c["KW"] == 3 for c in cs)
    assert any(c["KW"] * c["Cin"] == 2816 for c in cs)
    assert any(c["in16"] and c["in_slope"] == 1.0 and not c["n_add"] for c in cs) and any(c["in16"] and c["in_slope"] == 0.25 and not c["n_add"] for c in cs)
    assert any(c["in16"] and c["in_slope"] == 0.1 for c in cs)                                       # the engine's staging slope
    assert {(c["n_add"], c["in_div"]) for c in cs if c["n_add"]} >= {(1, 1.0), (2, 1.0), (3, 1.0), (1, 3.0), (2, 3.0), (3, 3.0)}
    ep = {(c["act_slope"] != 1.0, c["res"], c["accumulate"], c["out_div"] != 1.0) for c in cs}
    assert ep >= {(False, False, False, False), (True, False, False, False), (True, True, False, False), (True, True, True, False),
                  (True, True, True, True), (False, True, True, True)}
    assert {0.1, 0.0} <= {c["act_slope"] for c in cs}
    assert {c["special"] for c in cs} == {None, "inf", "sub"}


def _vocoder_lines(dtype, w, b):
    """An Act16Vocoder (tests/act16_ref.py) around given 16-bit weights and biases, accumulating in float64."""
    import torch
    import act16_ref
    v = object.__new__(act16_ref.Act16Vocoder)
    v.hg, v.dtype, v.acc, v.drop = {"resblock": 1}, dtype, torch.float64, set()
    v.w = {k: torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))) for k, x in w.items()}      # [Cout, KW, Cin] -> [Cout, Cin, KW]
    v.b = {k: torch.from_numpy(x) for k, x in b.items()}
    return v


@pytest.mark.parametrize("kind", KINDS, ids=["bf16_act", "fp16_act"])
def test_act16_chain_and_stage_are_the_lines_of_act16_ref(kind):
    """One ResBlock1 pair of act16_ref.Act16Vocoder (torch casts: xt = r(lrelu(x)); r(c1 + b1); r(lrelu); r(c2 + b2); x = r(xt + x)) against
    two convolutions restated with act16_stage / act16_chain, and the stage sum (xs = r(xs + rb_j); x = r(xs / n); r(lrelu)) against the
    joined staging form.  Grid data (negatives on coarse values: the slope is 0.1) and float64 accumulation on both sides, so both sum exactly."""
    import torch
    dtype = torch.bfloat16 if kind == kr.A16_BF16 else torch.float16
    c1 = kc._acase("ref_c1", "", 2, 33, 32, 32, 3, 3, act_slope=0.1, **kc._NEG01)
    d1 = kr.a16_data(c1, kind)
    assert kr.act16_exactness(c1, kind, d1)[0] < kr.A16_EXACT_LIMIT
    h = kr.a16_exact(c1, kind, d1)                                     # r(lrelu(r(c1 + b1)))
    c2 = kc._acase("ref_c2", "", 2, 33, 32, 32, 3, 1, res=True, **kc._COARSE)
    d2 = dict(kr.a16_data(c2, kind), x=h, res=d1["x"])
    # conv2's input is no grid any more (r(0.1 v)), but 96 products of 16-bit values sum exactly in float64 on both sides; one rounding to float32
    second = lambda dd: kr.act16_chain(kr.a16_sum64(c2, kind, dd)[0].astype(np.float32), c2, dd["res"], None, kind)   # noqa: E731
    mine = second(d2)
    v = _vocoder_lines(dtype, {"resblocks.0.convs1.0": d1["w"], "resblocks.0.convs2.0": d2["w"]},
                       {"resblocks.0.convs1.0": d1["bias"], "resblocks.0.convs2.0": d2["bias"]})
    theirs = v._resblock(0, torch.from_numpy(np.ascontiguousarray(d1["x"].transpose(0, 2, 1))), 3, [3]).numpy().transpose(0, 2, 1)
    assert np.array_equal(kr.bits16(mine, kind), kr.bits16(theirs, kind))
    v.drop = {"c1"}                                                    # act16_ref's own mutation is the chain's 'drop_bias_round'
    dropped = v._resblock(0, torch.from_numpy(np.ascontiguousarray(d1["x"].transpose(0, 2, 1))), 3, [3]).numpy().transpose(0, 2, 1)
    pre1 = kr.a16_sum64(c1, kind, d1)[0].astype(np.float32)
    h_drop = kr.act16_chain(pre1, c1, None, None, kind, mut="drop_bias_round")
    assert np.array_equal(kr.bits16(second(dict(d2, x=h_drop)), kind), kr.bits16(dropped, kind))
    assert not np.array_equal(h_drop, h)
    # the stage sum and the next layer's activation: Gaussian 16-bit tensors
    r = v.r
    cj = kc._acase("ref_join", "", 2, 33, 32, 32, 1, n_add=2, in_div=3.0, in_slope=0.1)
    dj = kr.a16_data(cj, kind, "general")
    xs = [torch.from_numpy(t) for t in [dj["x"]] + dj["adds"]]
    want = r(xs[0] + xs[1])
    want = r(want + xs[2])
    want = r(want / 3)
    import act16_ref
    want = r(act16_ref.lrelu(want, 0.1)).numpy()
    assert np.array_equal(kr.bits16(kr.act16_stage(cj, kind, dj["x"], dj["adds"]), kind), kr.bits16(want, kind))
    assert np.array_equal(kr.act16_round(dj["w"], kind), r(torch.from_numpy(dj["w"])).numpy())
    big = np.array([65519.9, 65520.0, -1e6, 3e38, 2.0 ** -25, 2.0 ** -24 * 1.5, 2.0 ** -24 * 2.5, 1e-9], np.float32)   # overflow, subnormals, ties
    assert np.array_equal(kr.bits16(kr.act16_round(big, kind), kind), kr.bits16(r(torch.from_numpy(big)).numpy(), kind))


@pytest.mark.slow
@pytest.mark.parametrize("c", kc.A16_CASES, ids=lambda c: c["name"])
def test_a16_float32_evaluations_pass_both_tiers(c):
    """float32 evaluations in the three orders equal the exact tier's expectation bit for bit, and pass both rules of the general tier."""
    for kind in KINDS:
        d = kr.a16_data(c, kind)
        want = kr.bits16(kr.a16_exact(c, kind, d), kind)
        z = kr.a16_data(c, kind, "zero_mean")
        for order in ("blocked", "sequential", "matmul"):
            assert kr.check_a16_interval(c, kind, z, kr.a16_eval32(c, kind, z, order))[0] == 0, (c["name"], kind, order)
        cg = kr.a16_general_case(c)
        g = kr.a16_data(cg, kind, "general")
        ref = kr.a16_general_reference(cg, kind, g)
        yard = kr.flip_share(kr.a16_eval32(cg, kind, g), ref["mid"], kind)
        for order in ("blocked", "sequential", "matmul"):
            assert np.array_equal(kr.bits16(kr.a16_eval32(c, kind, d, order), kind), want), (c["name"], kind, order)
            rr = kr.check_a16_general(cg, kind, g, kr.a16_eval32(cg, kind, g, order), ref, yard)
            print(f"{c['name']} {kr.A16_NAME[kind]} {order}: flip share {rr['share']:.3g} (yardstick {rr['yard']:.3g}), one-value intervals {rr['one_value']:.3g}")
            assert rr["ok"], (c["name"], kind, order, rr["why"])


# the smallest case in which each mutation exists, and the K = 2816 one (the channel-tail mutation at 11 x 80 = 880, as above)
A16_MUT_SMALL = kc._acase("mut16_small", "", 2, 33, 8, 32, 3, n_add=2, in_slope=0.25, act_slope=0.1, res=True, accumulate=True, out_div=3.0)
A16_MUT_LARGE = kc._acase("mut16_k2816", "", 1, 65, 256, 128, 11, 5, n_add=2, ag={1: (96, -6), 2: (2047, -9)}, wg=(1, -6), fine16=False, in_slope=0.25, act_slope=0.1, res=True,
                          accumulate=True, out_div=3.0)
A16_MUT_LARGE_TAIL = kc._acase("mut16_k880", "", 1, 65, 80, 128, 11, 5, in_slope=0.25, act_slope=0.1, res=True)
A16_MUT_INF = kc.A16_BY_NAME["a_64x64_inf"]
A16_MUT_SUB = kc.A16_BY_NAME["a_64x64_sub"]
A16_MUT_LARGE_INF = dict(kc.A16_BY_NAME["a_32x128_long_k"], name="mut16_k2816_inf", xg=(48, 3), wg=(16, -1), fine16=False)
A16_MUT_LARGE_SUB = dict(kc.A16_BY_NAME["a_32x128_long_k"], name="mut16_k2816_sub", xg=(48, -24), wg=(16, -5), fine16=False)
# (mutation, cases, kinds, caught by the general tier as well -- on the first case, Gaussian data)
A16_MUTATIONS = [
    ("drop_bias_round", (A16_MUT_SMALL, A16_MUT_LARGE), KINDS),
    ("rtz", (A16_MUT_SMALL, A16_MUT_LARGE), KINDS),
    ("res_before_act", (A16_MUT_SMALL, A16_MUT_LARGE), KINDS),
    ("div_before", (A16_MUT_SMALL, A16_MUT_LARGE), KINDS),
    ("drop_join", (A16_MUT_SMALL, A16_MUT_LARGE, kc.A16_BY_NAME["a_256x32_t256_add2_div"]), KINDS),     # ... and on the in_div path
    ("drop_tap_last_row", (A16_MUT_SMALL, A16_MUT_LARGE), KINDS),
    ("tail_not_zeroed", (A16_MUT_SMALL, A16_MUT_LARGE_TAIL), KINDS),
    ("sat", (A16_MUT_INF, A16_MUT_LARGE_INF), [kr.A16_FP16]),
    ("ftz", (A16_MUT_SUB, A16_MUT_LARGE_SUB), [kr.A16_FP16]),
]


@pytest.mark.parametrize("mut,cases,kinds", A16_MUTATIONS, ids=[m[0] for m in A16_MUTATIONS])
def test_every_a16_mutation_fails_the_exact_tier(mut, cases, kinds):
    for c in cases:
        for kind in kinds:
            d = kr.a16_data(c, kind)
            assert kr.act16_exactness(c, kind, d)[0] < kr.A16_EXACT_LIMIT, (c["name"], kind)
            want = kr.bits16(kr.a16_exact(c, kind, d), kind)
            assert np.array_equal(kr.bits16(kr.a16_eval32(c, kind, d), kind), want)
            assert not np.array_equal(kr.bits16(kr.a16_eval32(c, kind, d, mut=mut), kind), want), (mut, c["name"], kind)


def test_a16_wrappers_and_groups_refuse_before_any_launch(kh):
    """The 16-bit launches and the group launchers validate on the host (made-up addresses: nothing reaches the GPU runtime)."""
    one = 4096
    c = kc.A16_BY_NAME["a_64x64_t63"]
    a = {k: v for k, v in _a16_host_args(c, kr.A16_BF16).items() if k != "rows_hint"}
    a = {k: (one if v == 16 else v) for k, v in a.items()}
    alone = "16-bit activations write the 16-bit output alone"
    assert alone in kh.conv_bf16(**dict(a, out=one)) and alone in kh.conv_bf16(**dict(a, outb_slope=0.5))
    assert alone in kh.conv_bf16(**dict(a, in_bf16=0, in_add0=one))                      # a join of fp32 inputs
    assert "act16 is 0" in kh.conv_bf16(**dict(a, act16=3))
    assert "front" in kh.conv_bf16(**dict(a, in_add1=one)) and "out_div needs accumulate" in kh.conv_bf16(**dict(a, accumulate=0))
    assert "needs an fp32 input" in kh.conv_bf16(**dict(a, act16=0, out=one, out_b=None, in_add0=one, res=None))
    share = "the members of a group share"
    assert share in kh.conv_bf16_group([a, dict(a, act16=kr.A16_FP16)]) and share in kh.conv_bf16_group([a, dict(a, T=c["T"] + 1)])
    assert share in kh.conv_bf16_group([a, dict(a, in_bf16=0)]) and "1 .. 4 members" in kh.conv_bf16_group([a] * 5)
    assert "unsupported shape" in kh.conv_bf16_group([a, dict(a, Cout=48)]) and alone in kh.conv_bf16_group([a, dict(a, out=one)])
    p = dict(x=one, b1=one, b2=one, out=2 * one, B=2, T=65, C=32, KW=3, dil=1, mode=3, bimg1=one, bimg2=one)
    assert share in kh.pair_bf16_group([p, dict(p, mode=4)]) and share in kh.pair_bf16_group([p, dict(p, C=64)])
    assert "in-place" in kh.pair_bf16_group([p, dict(p, out=one)]) and "out_div" in kh.pair_bf16_group([p, dict(p, out_div=3.0)])
    assert "unsupported" in kh.pair_bf16_group([p, dict(p, KW=4)]) and "1 .. 4 members" in kh.pair_bf16_group([p] * 5)
    assert "null pointer" in kh.conv_post_bf16(None, one, one, one, None, 1, 8, 32, 7) and "bad dims" in kh.conv_post_bf16(one, one, one, one, None, 1, 8, 30, 7)
    assert "bad dims" in kh.conv_post_bf16(one, one, one, one, None, 1, 8, 256, 7, fp16=True) and "8-byte aligned" in kh.conv_post_bf16(one + 4, one, one, one, None, 1, 8, 32, 7)


def _general_verdict(c, kind, mut):
    cg = kr.a16_general_case(c)
    g = kr.a16_data(cg, kind, "general")
    return kr.check_a16_general(cg, kind, g, kr.a16_eval32(cg, kind, g, mut=mut))


@pytest.mark.slow
def test_which_a16_mutations_the_general_tier_also_catches():
    """On Gaussian data the general tier catches every mutation of the list but the two that need fp16's range (the Gaussian data stays
    inside it): a saturated overflow and a flushed subnormal are left to the exact tier's 'inf' and 'sub' cases."""
    for mut, cases, kinds in A16_MUTATIONS:
        for kind in kinds:
            r = _general_verdict(cases[0], kind, mut)
            assert r["ok"] == (mut in ("sat", "ftz")), (mut, kind, r)


def test_a_wrong_tie_rule_needs_the_exact_tier():
    """What the exact tier is for.  Ties sent away from zero instead of to even, fp16, a convolution with its bias alone: the grid data's
    sums are exact ties in a tenth of the elements, and the exact tier fails on each; a Gaussian sum is never a tie, so the general tier
    sees the float32 yardstick's own share of flips, no element outside its interval, and passes."""
    c, kind = kc._acase("rha_bias_only", "", 2, 65, 32, 64, 3), kr.A16_FP16
    d = kr.a16_data(c, kind)
    assert kr.act16_exactness(c, kind, d)[0] < kr.A16_EXACT_LIMIT
    differ = np.mean(kr.bits16(kr.a16_eval32(c, kind, d, mut="rha"), kind) != kr.bits16(kr.a16_exact(c, kind, d), kind))
    assert differ > 0.02, differ
    r = _general_verdict(c, kind, "rha")
    assert r["ok"] and r["outside"] == 0, r
