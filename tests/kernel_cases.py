"""The case matrix of the kernel-level differential tests, as data: tests/test_kernel_ref_host.py (CPU) checks it, and the GPU module that
launches these cases through tests/kernel_harness.py imports the same lists.  A case fixes the launch; its inputs come from a numpy generator seeded by the case's name (kernel_ref.conv_data ...).

Convolutions.  Not the full product of the axes: every value of every axis appears, and so does every pair of values that share code --
tile edge (T % 32 / 64 / 128 / 256 in {0, 1, BM - 1}, Cout % 32) x epilogue kind (vector / scalar, residual, accumulate, lens), and chunk
tail (Cin % 32 in {0, 4, 16}) x kernel size.  `reach` names the variant a case is there for; test_kernel_ref_host.py checks the predicates
that select it (variant() below restates launch_conv_gemm's choice), so a later change of the tile choice fails there instead of silently
dropping coverage."""
from __future__ import annotations

ACT_NONE, ACT_RELU, ACT_TANH, ACT_LRELU, ACT_SWISH, ACT_GELU = 0, 1, 2, 3, 4, 5
MAX_HALO = 64
KS_MAX_HALO = 16       # conv_ksplit / conv_rows
ROWMAP_MAX = 64


def _case(name, B, T, Cin, Cout, KW=1, dil=1, pad="c", **o):
    """pad: 'c' centred, '0' none, 'L' everything on the left (ffn_padding LEFT)."""
    halo = dil * (KW - 1)
    c = dict(name=name, B=B, T=T, Cin=Cin, Cout=Cout, KW=KW, dil=dil, pad={"c": halo // 2, "0": 0, "L": halo}[pad],
             wfrag=False, bias=False, res=False, lens=None, act_rows=None, host=False, accumulate=False, out_div=1.0, in_slope=1.0,
             act=ACT_NONE, act_slope=0.0, zts=0, in_pad=4, out_pad=4, res_pad=8, env=None, reach=None)
    bad = set(o) - set(c)
    assert not bad, bad
    c.update(o)
    return c


def _ragged(B, T, seed):
    """B row counts in [0, T]: the first is T, the second 0 (when B >= 2), then a fixed pseudo-random spread."""
    r = [T, 0] + [(seed * 7919 + 104729 * i) % (T + 1) for i in range(B)]
    return r[:B]


CONV_CASES = [
    # ---- tile and chunk edges, epilogue kinds (small launches: Cout > 64 -> the 64 x 64 tile, else 256 x 64 / 256 x 32)
    _case("t1_c1", 1, 1, 4, 1, reach=dict(scalar=True)),
    _case("t2_c2_k3", 2, 2, 4, 2, 3, bias=True, reach=dict(scalar=True)),
    _case("t63_c18_k3d5", 3, 63, 36, 18, 3, 5, bias=True, res=True, lens=[63, 0, 31], reach=dict(scalar=True)),
    _case("t64_c32_k7", 2, 64, 32, 32, 7, bias=True, act=ACT_RELU, reach=dict(cls=("conv_gemm_256x32", "conv_x3_256x32"), bfrag=False)),
    _case("t65_c33_k9", 2, 65, 80, 33, 9, bias=True, res=True, act=ACT_LRELU, act_slope=0.2, lens=[65, 64], reach=dict(scalar=True)),
    _case("t127_c64_k11d5", 2, 127, 36, 64, 11, 5, bias=True, in_slope=0.1, reach=dict(cls=("conv_gemm_256x64", "conv_x3_256x64"), bfrag=False)),
    _case("t128_c80_k3", 3, 128, 128, 80, 3, wfrag=True, bias=True, act=ACT_TANH, lens=[128, 1, 127],
          reach=dict(cls=("conv_gemm_64x64", "conv_x3_64x64"), bfrag=True, cpi=0)),
    _case("t129_c96_halo64", 2, 129, 32, 96, 9, 8, pad="0", wfrag=True, res=True, reach=dict(cls=("conv_gemm_64x64", "conv_x3_64x64"), bfrag=True)),
    _case("t255_c128_k3_left", 2, 255, 192, 128, 3, pad="L", wfrag=True, bias=True, res=True, act=ACT_RELU, reach=dict(bfrag=True)),
    _case("t257_c130_k1", 2, 257, 256, 130, bias=True, act=ACT_SWISH, reach=dict(scalar=True)),
    _case("t257_c256_k7_nofrag", 1, 257, 36, 256, 7, bias=True, lens=[129], reach=dict(cls=("conv_gemm_64x64", "conv_x3_64x64"), bfrag=False)),
    _case("t65_c128_k11_c256", 1, 65, 256, 128, 11, wfrag=True, bias=True, res=True),   # the longest K of the matrix: 2816
    _case("t65_c128_k11d5_c80", 2, 65, 80, 128, 11, 5, wfrag=True, in_slope=0.1, act=ACT_LRELU, act_slope=0.1),
    _case("t129_c64_k7_left", 2, 129, 80, 64, 7, pad="L", bias=True, act=ACT_SWISH),
    _case("t63_c32_k9_pad0", 2, 63, 128, 32, 9, pad="0", bias=True, act=ACT_TANH, lens=[62, 63]),
    _case("t513_c2_k3d5", 1, 513, 32, 2, 3, 5, res=True, accumulate=True, out_div=3.0, reach=dict(scalar=True, accumulate=True)),
    _case("t64_c384_k3", 2, 64, 36, 384, 3, wfrag=True, bias=True),
    # ---- plain Linear layers on the fragment path: 4, 2 and 1 chunks per work item
    _case("lin_cpi4", 1, 513, 256, 256, wfrag=True, bias=True, reach=dict(cls=("conv_gemm_64x64", "conv_x3_64x64"), bfrag=True, cpi=4)),
    _case("lin_cpi2", 2, 129, 192, 384, wfrag=True, res=True, lens=[129, 64], reach=dict(bfrag=True, cpi=2)),
    _case("lin_cpi0", 2, 65, 80, 96, wfrag=True, bias=True, reach=dict(bfrag=True, cpi=0)),
    _case("lin_cpi4_t127", 3, 127, 128, 80, wfrag=True, act=ACT_RELU, act_rows=[127, 64, 1], reach=dict(bfrag=True, cpi=4)),
    # ---- accumulate / out_div, input activation
    _case("acc_div3_frag", 2, 129, 32, 128, 3, wfrag=True, bias=True, accumulate=True, out_div=3.0, in_slope=0.1,
          reach=dict(bfrag=True, accumulate=True, cpi=0)),
    _case("acc_c64", 2, 257, 36, 64, 3, 5, bias=True, accumulate=True, reach=dict(cls=("conv_gemm_256x64", "conv_x3_256x64"), accumulate=True)),
    _case("acc_lin_frag", 2, 128, 128, 96, wfrag=True, accumulate=True, out_div=3.0, lens=[128, 100], reach=dict(bfrag=True, accumulate=True, cpi=0)),
    # ---- GELU (fp32 and bf16x3 only)
    _case("gelu_frag", 2, 129, 36, 96, 9, wfrag=True, bias=True, act=ACT_GELU, reach=dict(gelu=True, bfrag=True)),
    _case("gelu_c64", 2, 257, 80, 64, 9, bias=True, act=ACT_GELU, lens=[257, 130], reach=dict(gelu=True, bfrag=False)),
    _case("gelu_scalar", 2, 65, 32, 18, 3, bias=True, act=ACT_GELU, reach=dict(gelu=True, scalar=True)),
    # ---- ragged batches: act_rows alone (padded grid), with the host copy (compact grid; B = 70 exceeds the table: padded fallback)
    _case("rows_dev", 3, 257, 32, 96, 3, wfrag=True, bias=True, act_rows=[257, 0, 100]),
    _case("rows_host_b1", 1, 255, 36, 128, 3, wfrag=True, act_rows=[130], host=True),
    _case("rows_host_b3", 3, 129, 32, 33, 7, bias=True, res=True, act_rows=[129, 0, 65], host=True, reach=dict(scalar=True)),
    _case("rows_host_b64", 64, 63, 32, 64, 3, bias=True, act_rows=_ragged(64, 63, 1), host=True, lens=_ragged(64, 63, 1)),
    _case("rows_host_b70", 70, 65, 4, 96, 3, wfrag=True, act_rows=_ragged(70, 65, 2), host=True),
    # ---- structural zeros of a polyphase upsampler
    _case("zts32_c64", 2, 257, 32, 64, 3, wfrag=True, bias=True, zts=32, reach=dict(cls=("conv_gemm_256x32", "conv_x3_256x64"), narrow=True)),
    _case("zts48_c96", 2, 129, 36, 96, 3, wfrag=True, bias=True, zts=48, reach=dict(bfrag=True)),
    _case("zts128_c256", 1, 255, 32, 256, 3, wfrag=True, zts=128, reach=dict(bfrag=True)),
    # ---- launch sizes that select the large tiles (Cin small: the float64 reference stays cheap)
    _case("big_128x128_occ3", 64, 512, 32, 256, 3, wfrag=True, bias=True, res=True,
          reach=dict(cls=("conv_gemm_128x128", "conv_x3_128x128"), bfrag=True, occ3=True)),
    _case("big_128x128_lds", 64, 512, 4, 130, 3, bias=True, reach=dict(cls=("conv_gemm_128x128", "conv_x3_128x128"), scalar=True)),
    _case("big_128x128_nofrag", 64, 513, 32, 256, lens=_ragged(64, 513, 3), reach=dict(cls=("conv_gemm_128x128", "conv_x3_128x128"), bfrag=False)),
    _case("big_128x128_cpi4", 64, 512, 128, 256, wfrag=True, bias=True, reach=dict(cls=("conv_gemm_128x128", "conv_x3_128x128"), bfrag=True, cpi=4)),
    _case("big_64x128_under_round", 12, 513, 32, 256, 3, wfrag=True, bias=True, act=ACT_LRELU, act_slope=0.1,
          reach=dict(cls=("conv_gemm_64x128", "conv_x3_64x128"), bfrag=True)),
    _case("big_64x128_half", 32, 1152, 32, 256, wfrag=True, res=True, reach=dict(cls=("conv_gemm_64x128", "conv_x3_64x128"), bfrag=True, cpi=0)),
    _case("big_64x64_many_rows_nofrag", 12, 513, 32, 132, 3, bias=True, reach=dict(cls=("conv_gemm_64x64", "conv_x3_64x64"), bfrag=False)),
    _case("big_256x64", 8, 1025, 32, 64, 7, bias=True, res=True, reach=dict(cls=("conv_gemm_256x64", "conv_x3_256x64"))),
    _case("big_256x32", 8, 1025, 36, 32, 3, 5, bias=True, reach=dict(cls=("conv_gemm_256x32", "conv_x3_256x32"))),
    # ---- child process with E2ETTS_WG_PER_CU=1: the persistent multi-tile loop (tpb > 1, tile counts tpb does not divide)
    _case("wg1_64x128", 8, 2100, 32, 256, 3, wfrag=True, bias=True, env="wg1", reach=dict(cls=("conv_gemm_64x128", "conv_x3_64x128"), tpb=2)),
    _case("wg1_64x64_lds", 8, 2100, 36, 256, 3, bias=True, res=True, env="wg1", reach=dict(cls=("conv_gemm_64x64", "conv_x3_64x64"), tpb=4)),
    _case("wg1_128x128_acc", 32, 1100, 32, 256, 3, wfrag=True, accumulate=True, out_div=3.0, env="wg1",
          reach=dict(cls=("conv_gemm_128x128", "conv_x3_128x128"), tpb=2, accumulate=True)),
    _case("wg1_256x64_ragged", 64, 4200, 32, 64, 3, bias=True, act_rows=_ragged(64, 4200, 5), host=True, env="wg1",
          reach=dict(cls=("conv_gemm_256x64", "conv_x3_256x64"), tpb=2)),
    # ---- child process with E2ETTS_FRAG64=0: the 64 x 64 tile on the LDS weight tile although fragment-order weights are given
    _case("frag64off", 2, 129, 36, 96, 3, wfrag=True, bias=True, res=True, env="frag64"),
    _case("frag64off_acc", 2, 65, 80, 128, 7, wfrag=True, accumulate=True, out_div=3.0, env="frag64"),
]
CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)

ALL_CONV_CLASSES = {f"conv_{m}_{t}" for m in ("gemm", "x3") for t in ("256x32", "256x64", "64x64", "64x128", "128x128")}
# att_serial: the launcher never takes the split attention kernels, so the head dims that have a split form run on attention_kernel<dk> /
# attention_x3_kernel<dk, 8> (test_attention_serial_form_gives_the_split_forms_bits)
ENV_OF = {"wg1": {"E2ETTS_WG_PER_CU": "1"}, "frag64": {"E2ETTS_FRAG64": "0"}, "att_serial": {"E2ETTS_ATT_SPLIT_MAX": "0"}}


def modes_of(c):
    """The arithmetic modes a case runs in (ACT_GELU serves fp32 and bf16x3 only)."""
    return (0, 1) if c["act"] == ACT_GELU else (0, 1, 2)


# ---- launch_conv_gemm's choice, restated from conv_gemm.hip / host_logic.h (default environment)
def _counts(c):
    if c["act_rows"] is not None and c["host"]:
        v = [min(max(r, 0), c["T"]) for r in c["act_rows"]]
        return sum((r + 127) // 128 for r in v) * ((c["Cout"] + 127) // 128), sum(v)
    return c["B"] * ((c["T"] + 127) // 128) * ((c["Cout"] + 127) // 128), c["B"] * c["T"]


def epilogue_vec_ok(c):
    out_ld, res_ld = c["Cout"] + c["out_pad"], c["Cout"] + c["res_pad"]
    return c["Cout"] % 4 == 0 and out_ld % 4 == 0 and (not c["res"] or res_ld % 4 == 0)


def variant(c, x3, wg_per_cu=24, frag64=True):
    """(class string, dict(tile, bfrag, cpi, occ3, accumulate, scalar, gelu, narrow, tpb)) of launch_conv_gemm for the case in mode x3."""
    t128, rows = _counts(c)
    Cout, wfrag = c["Cout"], c["wfrag"]
    many = rows >= 6144
    few_n = Cout > 64 and t128 < 512 and not many
    under = Cout > 64 and t128 < 512 and many
    few = few_n or (not wfrag and under)
    half = False
    if wfrag:
        if under:
            half = True
        elif not c["accumulate"] and Cout > 64 and not few_n:
            half = t128 < 512 or 0.5 * 1.06 * ((2 * t128 + 511) // 512) < (t128 + 511) // 512
    narrow = x3 == 0 and c["zts"] == 32 and Cout == 64 and c["KW"] == 3 and wfrag and not c["accumulate"] and not c["res"]
    by_cout = "128x128" if Cout > 64 else ("256x64" if Cout > 32 else "256x32")
    if narrow:
        cls = "conv_gemm_256x32"
    else:
        tile = "64x64" if few else ("64x128" if half else by_cout)
        if not x3 and Cout <= 64:
            tile = by_cout
        cls = ("conv_x3_" if x3 else "conv_gemm_") + tile
    gelu = c["act"] == ACT_GELU
    scalar = not epilogue_vec_ok(c)
    if scalar:
        tile, bfrag, cpi, occ3 = "128x128", False, 0, False
    elif narrow:
        tile, bfrag, cpi, occ3 = "256x32", True, 0, False
    else:
        tile = cls.split("_")[-1]
        fragtile = tile in ("128x128", "64x128", "64x64")
        bfrag = bool(wfrag) and fragtile and not (tile == "64x64" and not frag64)
        cpi = 0
        if bfrag and not gelu and c["KW"] == 1 and not c["accumulate"]:
            cpi = 4 if c["Cin"] % 128 == 0 else (2 if c["Cin"] % 64 == 0 else 0)
        occ3 = bfrag and not gelu and cpi == 0 and x3 == 0 and tile == "128x128" and c["zts"] == 0
    BM, BN = (int(v) for v in tile.split("x"))
    mt, nt = (c["T"] + BM - 1) // BM, (Cout + BN - 1) // BN
    if c["act_rows"] is not None and c["host"] and c["B"] <= ROWMAP_MAX:
        total = sum((min(max(r, 0), c["T"]) + BM - 1) // BM for r in c["act_rows"]) * nt
    else:
        total = mt * nt * c["B"]
    tpb = min(max(total // (256 * wg_per_cu), 1), 64, mt)
    return cls, dict(tile=tile, bfrag=bfrag, cpi=cpi, occ3=occ3, accumulate=bool(c["accumulate"]), scalar=scalar, gelu=gelu, narrow=narrow, tpb=tpb)


def ksplit_ok(c, x3):
    return bool(c["wfrag"] and x3 == 0 and not c["accumulate"] and c["in_slope"] == 1.0 and c["zts"] == 0 and c["dil"] * (c["KW"] - 1) <= KS_MAX_HALO)


def rows_ok(c, x3):
    return bool(c["wfrag"] and not c["accumulate"] and c["out_div"] == 1.0 and c["in_slope"] == 1.0 and c["zts"] == 0
                and c["dil"] * (c["KW"] - 1) <= KS_MAX_HALO)


# conv_bf16 (plain bf16 = mode 2; dense rows, Cout % 32 == 0, Cin % 8 == 0): one case per tile shape bc_choose can return in the default
# environment (32 MT WGM x 32 WGN: wavefronts side by side on 128 / 64 / 32 columns, MT = 1 / 2 / 4 by the number of workgroups), options spread
def _bcase(name, cls, *a, **o):
    return _case(name, *a, in_pad=0, out_pad=0, res_pad=0, reach=dict(bcls=cls), **o)


BCONV_CASES = [
    _bcase("b_128x32", "conv_bf16_128x32", 2, 65, 32, 32, 3, bias=True, in_slope=0.1),
    _bcase("b_256x32", "conv_bf16_256x32", 16, 1025, 8, 32, 3, 5, bias=True, res=True),
    _bcase("b_512x32", "conv_bf16_512x32", 16, 513, 40, 96, bias=True, act=ACT_RELU),
    _bcase("b_64x64", "conv_bf16_64x64", 3, 129, 64, 64, 7, 3, bias=True, res=True, in_slope=0.1),
    _bcase("b_128x64", "conv_bf16_128x64", 16, 513, 32, 64, 3, bias=True, accumulate=True, out_div=3.0, in_slope=0.1),
    _bcase("b_256x64", "conv_bf16_256x64", 16, 1025, 32, 64, 3, bias=True, res=True, in_slope=0.1),
    _bcase("b_32x128", "conv_bf16_32x128", 1, 257, 128, 128, 11, bias=True, res=True, act=ACT_LRELU, act_slope=0.1, accumulate=True, out_div=3.0),
    _bcase("b_64x128", "conv_bf16_64x128", 8, 513, 32, 128, 3, 1, "L", bias=True),
    _bcase("b_128x128", "conv_bf16_128x128", 8, 513, 32, 256, 3, bias=True, in_slope=0.1),
    _bcase("b_long_k", "conv_bf16_32x128", 1, 513, 256, 256, 3, 5, in_slope=0.1),
    _bcase("b_poly", "conv_bf16_32x128", 2, 127, 64, 128, 3, bias=True, in_slope=0.1, zts=64),
    _bcase("b_halo64", "conv_bf16_64x64", 2, 129, 32, 64, 9, 8, "0", bias=True),
]
ALL_BCONV_CLASSES = {f"conv_bf16_{m}x{n}" for n, ms in ((128, (32, 64, 128)), (64, (64, 128, 256)), (32, (128, 256, 512))) for m in ms}

# ---- attention: (name, B, N, n_head, dk, lens or None, lens_host, workspace)
def _att(name, B, N, n_head, dk, lens=None, host=False, ws=False):
    return dict(name=name, B=B, N=N, n_head=n_head, dk=dk, lens=lens, host=host, ws=ws)


ATT_CASES = [
    _att("n1_dk32", 1, 1, 2, 32, [1]),
    _att("n31_dk64", 3, 31, 2, 64, [31, 0, 1]),
    _att("n32_dk96", 3, 32, 1, 96, [32, 31, 16]),
    _att("n33_dk128", 3, 33, 2, 128, [33, 32, 16], host=True),
    _att("n63_dk192", 1, 63, 1, 192, [62]),
    _att("n65_dk32", 3, 65, 2, 32, [65, 0, 32], host=True),
    _att("n255_dk64", 3, 255, 2, 64, [255, 254, 127], host=True),
    _att("n256_dk96", 1, 256, 2, 96, [256]),
    _att("n257_dk128", 3, 257, 1, 128, [257, 1, 128]),
    _att("n600_dk192", 1, 600, 1, 192, [599]),
    _att("n257_dk64_ws", 1, 257, 2, 64, [257], ws=True),
    _att("n600_dk64_ws", 3, 600, 2, 64, [600, 300, 1], ws=True),
    _att("n600_dk128_ws", 1, 600, 1, 128, [599], ws=True),
    _att("n257_dk192_ws", 1, 257, 1, 192, None, ws=True),
    _att("n63_dk64_nolens", 3, 63, 2, 64, None),
    _att("b40_n257_dk64", 40, 257, 4, 64, [257 - 6 * i for i in range(40)]),     # x3: 5 * 4 * 40 = 800 > 512 workgroups -> attention_x3_kernel<64, 8>
    _att("b40_n65_dk128_host", 40, 65, 8, 128, [(7 * i) % 66 for i in range(40)], host=True),
]

ATT_SPLIT_DK = (64, 128, 192)   # the head dims at which launch_attention has a split form

# ---- rel_attention: (name, B, N, n_head, dk, pos_rows); run with and without pos_x3 where the split form has the head dim
REL_CASES = [
    dict(name="r_n1_dk8", B=2, N=1, n_head=2, dk=8, pos_rows=4),
    dict(name="r_n2_dk16", B=2, N=2, n_head=2, dk=16, pos_rows=2),
    dict(name="r_n127_dk32", B=2, N=127, n_head=2, dk=32, pos_rows=200),
    dict(name="r_n128_dk48", B=1, N=128, n_head=2, dk=48, pos_rows=128),
    dict(name="r_n129_dk64", B=2, N=129, n_head=1, dk=64, pos_rows=130),
    dict(name="r_n300_dk96", B=1, N=300, n_head=1, dk=96, pos_rows=301),
    dict(name="r_n300_dk16", B=1, N=300, n_head=4, dk=16, pos_rows=512),
    dict(name="r_n129_dk8", B=1, N=129, n_head=4, dk=8, pos_rows=129),
]
REL_X3_DK = (16, 32, 48, 64, 96)

LN_CASES = [dict(name=f"ln_c{C}", B=3, N=N, C=C, lens=lens) for C, N, lens in ((4, 5, None), (80, 33, [33, 0, 17]), (256, 65, [65, 64, 1]), (1024, 9, None))]

POST_CASES = [
    dict(name="post_c4", B=2, N=300, C=4, KW=7, n_add=0, x_div=1.0, act_rows=None, host=False),
    dict(name="post_c32_add1", B=3, N=513, C=32, KW=7, n_add=1, x_div=2.0, act_rows=[513, 0, 257], host=True),
    dict(name="post_c128_add3", B=2, N=1000, C=128, KW=7, n_add=3, x_div=3.0, act_rows=[1000, 300], host=False),
    dict(name="post_c32_add2", B=1, N=255, C=32, KW=7, n_add=2, x_div=3.0, act_rows=None, host=False),
]
DW_CASES = [dict(name=f"dw_c{C}_k{k}", B=2, N=N, C=C, k=k) for C, k, N in ((4, 3, 5), (64, 7, 129), (128, 15, 65), (128, 31, 200), (256, 31, 63), (80, 31, 64), (32, 7, 70))]
DW_FUSED = lambda C, k: (k == 31 and C % 128 == 0) or (k == 15 and C % 128 == 0) or (k == 7 and C % 64 == 0)   # noqa: E731
GLU_CASES = [dict(name=f"glu_c{C}", rows=rows, C=C) for rows, C in ((1, 4), (77, 80), (513, 256))]

# ---- fused ResBlocks: pairs (resblock_pair in modes 0 / 1 / 2, pair_bf16) and kernel-size-3 chains (resblock_chain, rb_bf16, rb_bf16_stage)
PAIR_CASES = [
    dict(name="pair_c32_k3d1", B=2, T=300, C=32, KW=3, dil=1, accumulate=False, out_div=1.0),
    dict(name="pair_c64_k3d5", B=2, T=513, C=64, KW=3, dil=5, accumulate=True, out_div=3.0),
    dict(name="pair_c128_k7d3", B=1, T=257, C=128, KW=7, dil=3, accumulate=False, out_div=1.0),
    dict(name="pair_c256_k11d5", B=1, T=129, C=256, KW=11, dil=5, accumulate=True, out_div=1.0),
]
CHAIN_CASES = [
    dict(name="chain_c32", B=2, T=700, C=32, KW=3, dil=[1, 3, 5], accumulate=False, out_div=1.0),
    dict(name="chain_c64_acc", B=1, T=513, C=64, KW=3, dil=[1, 3, 5], accumulate=True, out_div=3.0),
]


# ---- conv_bf16 with 16-bit activations (BConvParams::act16 = 1 bf16, 2 fp16; every case runs at both).  Small launches: the large tiles are
# reached through rows_hint (bc_choose counts it instead of B x T).  in16: the input is a 16-bit tensor (else fp32: conv_pre taking the
# mel); n_add / in_div: the join of 16-bit inputs; act_slope: 1.0 = none.  The exact tier's data grids (kernel_ref.a16_grids): xg / wg / ag
# = (kmax, exponent) of x, w and the addends, neg = the negatives x may take (a non-dyadic staging slope), fb = bits an fp32 input carries
# past the element type, fine16 = the fp16 grids are finer by 2^-2.  special: 'inf' -- sums past 65504, which fp16 must turn into
# infinities; 'sub' -- inputs and results that are fp16 subnormals.  kmin: the smallest |k| of the x grid (a join with in_div whose
# roundings change the sums: x far from zero keeps the lowest set bit of r(x / 3) coarse, the addends' finer grid makes r(in + a) round).
def _acase(name, cls, B, T, Cin, Cout, KW=1, dil=1, pad="c", in16=True, n_add=0, in_div=1.0, rows_hint=0, act_slope=1.0, xg=(48, -4), wg=(16, -6),
           ag=None, neg=None, fb=None, fine16=True, special=None, kmin=0, **o):
    c = _case(name, B, T, Cin, Cout, KW, dil, pad, in_pad=0, out_pad=0, res_pad=0, reach=dict(bcls=cls), bias=True, **o)
    c.update(in16=in16, n_add=n_add, in_div=in_div, rows_hint=rows_hint, act_slope=act_slope, xg=xg, wg=wg, ag=ag, neg=neg, fb=fb, fine16=fine16,
             special=special, kmin=kmin)
    assert in16 or not n_add
    return c


_ENGINE = dict(res=True, accumulate=True, out_div=3.0)                      # the engine's own combination: residual + sum + division
_COARSE = dict(xg=(6, 0), wg=(4, -6), ag=(6, 0), fine16=False)                        # integers: what a division by 3 or a slope of 0.1 can still sum exactly
_NEG01 = dict(in_slope=0.1, neg=(-1, -2, -4), **_COARSE)                    # the engine's staging slope on 16-bit inputs
A16_CASES = [
    # ---- 128 x 32 (Cout % 64 != 0, few rows)
    _acase("a_128x32_t1", "conv_bf16_128x32", 2, 1, 8, 32, 3, **_NEG01),
    _acase("a_128x32_t31", "conv_bf16_128x32", 3, 31, 40, 96, 3, 5, in16=False, in_slope=0.25, act_slope=0.1),
    _acase("a_128x32_t33_pre", "conv_bf16_128x32", 2, 33, 80, 32, 7, in16=False),                                   # conv_pre taking the mel
    _acase("a_128x32_t127", "conv_bf16_128x32", 2, 127, 32, 32, 3, act_slope=0.0, res=True),
    _acase("a_128x32_t128", "conv_bf16_128x32", 1, 128, 32, 96, 3, 1, "L", in_slope=0.25, act_slope=0.1, res=True, accumulate=True),
    _acase("a_128x32_t129_add1", "conv_bf16_128x32", 2, 129, 8, 32, 3, n_add=1, in_slope=0.25, act_slope=0.1, **_ENGINE),
    # ---- 256 x 32
    _acase("a_256x32_t255", "conv_bf16_256x32", 1, 255, 40, 32, 3, 5, in16=False, in_slope=0.25, rows_hint=12288, **_ENGINE),
    _acase("a_256x32_t256_add2_div", "conv_bf16_256x32", 1, 256, 8, 32, 3, n_add=2, in_div=3.0, in_slope=0.25, rows_hint=12288,
           xg=(48, 0), kmin=32, wg=(4, -6), ag={1: (48, -4), 2: (384, -7)}, fine16=False),        # the join's roundings bite here
    _acase("a_256x32_t257", "conv_bf16_256x32", 1, 257, 64, 32, act_slope=0.0, in_slope=0.25, rows_hint=12288),
    # ---- 512 x 32
    _acase("a_512x32_t511", "conv_bf16_512x32", 1, 511, 8, 32, 3, act_slope=0.1, res=True, rows_hint=32768),
    _acase("a_512x32_t512", "conv_bf16_512x32", 1, 512, 32, 32, 3, 1, "L", in16=False, rows_hint=32768),
    _acase("a_512x32_t513", "conv_bf16_512x32", 1, 513, 40, 32, 3, in_slope=0.25, rows_hint=32768, **_ENGINE),
    # ---- 64 x 64
    _acase("a_64x64_t33_add3_div", "conv_bf16_64x64", 3, 33, 8, 64, 3, n_add=3, in_div=3.0, in_slope=0.25, act_slope=0.1, **_ENGINE, **_COARSE),
    _acase("a_64x64_t63", "conv_bf16_64x64", 2, 63, 64, 64, 7, 3, in_slope=0.25, act_slope=0.1, **_ENGINE),
    _acase("a_64x64_t64_halo64", "conv_bf16_64x64", 2, 64, 32, 64, 9, 8, "0", in16=False, in_slope=0.25),
    _acase("a_64x64_t65", "conv_bf16_64x64", 2, 65, 80, 64, 7, in16=False, act_slope=0.1),
    _acase("a_64x64_inf", "conv_bf16_64x64", 2, 65, 32, 64, 3, xg=(48, 4), wg=(16, 0), fine16=False, special="inf", act_slope=0.1, **_ENGINE),
    _acase("a_64x64_sub", "conv_bf16_64x64", 2, 65, 32, 64, 3, xg=(48, -24), wg=(16, -3), fine16=False, special="sub", in_slope=0.25, act_slope=0.1,
           res=True),
    # ---- 128 x 64
    _acase("a_128x64_t127", "conv_bf16_128x64", 1, 127, 32, 64, 3, in16=False, in_slope=0.25, act_slope=0.0, res=True, rows_hint=6144),
    _acase("a_128x64_t128_add3", "conv_bf16_128x64", 1, 128, 8, 64, 3, n_add=3, in_slope=0.25, rows_hint=6144),
    _acase("a_128x64_t129", "conv_bf16_128x64", 2, 129, 64, 64, 3, 5, **_ENGINE, rows_hint=6144),
    # ---- 256 x 64
    _acase("a_256x64_t255_add1_div", "conv_bf16_256x64", 1, 255, 8, 64, 3, n_add=1, in_div=3.0, in_slope=0.25, rows_hint=12288, **_COARSE),
    _acase("a_256x64_t256", "conv_bf16_256x64", 1, 256, 32, 64, 3, in16=False, in_slope=0.25, act_slope=0.1, res=True, accumulate=True, rows_hint=12288),
    _acase("a_256x64_t257", "conv_bf16_256x64", 1, 257, 32, 64, 3, 1, "0", in_slope=0.25, act_slope=0.1, rows_hint=12288),
    # ---- 32 x 128
    _acase("a_32x128_t1", "conv_bf16_32x128", 3, 1, 32, 128, 3, in16=False, in_slope=0.25, act_slope=0.1),
    _acase("a_32x128_t31_add2", "conv_bf16_32x128", 2, 31, 8, 128, 3, n_add=2, in_slope=0.25, res=True),
    _acase("a_32x128_t32", "conv_bf16_32x128", 2, 32, 32, 256, 3, act_slope=0.1, **_ENGINE),
    _acase("a_32x128_t33_s01", "conv_bf16_32x128", 2, 33, 32, 128, 3, act_slope=0.1, res=True, **_NEG01),
    _acase("a_32x128_poly", "conv_bf16_32x128", 2, 127, 64, 128, 3, in_slope=0.25, zts=64),
    _acase("a_32x128_long_k", "conv_bf16_32x128", 1, 129, 256, 128, 11, 5, in_slope=0.25, act_slope=0.1, **_ENGINE),   # the longest K of the matrix: 2816
    # ---- 64 x 128
    _acase("a_64x128_t63", "conv_bf16_64x128", 1, 63, 32, 128, 3, in16=False, in_slope=0.25, res=True, rows_hint=3072),
    _acase("a_64x128_t64", "conv_bf16_64x128", 1, 64, 256, 128, 3, in_slope=0.25, act_slope=0.1, rows_hint=3072),
    _acase("a_64x128_t65", "conv_bf16_64x128", 2, 65, 32, 128, 7, 1, "L", **_ENGINE, rows_hint=3072),
    # ---- 128 x 128
    _acase("a_128x128_t127", "conv_bf16_128x128", 1, 127, 32, 256, 3, in_slope=0.25, act_slope=0.0, rows_hint=3072),
    _acase("a_128x128_t128", "conv_bf16_128x128", 1, 128, 32, 128, 3, in16=False, in_slope=0.25, act_slope=0.1, **_ENGINE, rows_hint=6144),
    _acase("a_128x128_t129", "conv_bf16_128x128", 2, 129, 32, 128, 3, 5, in_slope=0.25, res=True, rows_hint=6144),
]
A16_BY_NAME = {c["name"]: c for c in A16_CASES}
assert len(A16_BY_NAME) == len(A16_CASES)
A16_BM = lambda c: int(c["reach"]["bcls"].split("_")[-1].split("x")[0])   # noqa: E731  -- rows of the tile a case names
