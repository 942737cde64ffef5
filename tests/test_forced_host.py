"""The teacher-forced pass without a GPU: the numpy restatement (tests/forced_ref.py) against every fixture the reference generated
(tools/make_forced_goldens.py), frame2phoneme with its in-place quirk against its direct fixture, the new symbol in its header / export map /
binding / library, and e2etts_acoustic_forced's argument checks (csrc/host_logic.h: forced_check) as a stand-alone program under ASan + UBSan.

Bars: discrete outputs and uv exact; float arrays <= 1e-5 mean-L1 (the oracle's bar), or twice the module's own recorded fp32-vs-float64
distance where that is larger (as tests/test_fastformer_host.py does)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import forced_cases as fc
import forced_ref as fr
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "forced_logic_test.cc")


@pytest.mark.parametrize("name", fc.MODEL_FIXTURES)
def test_restatement_against_the_reference_fixture(name):
    from e2e_tts_amd.packer import variance_position_table
    g = fc.load(name)
    cfg, state, _ = fc.states_of(g)
    fs = cfg["models"]["fastspeech2"]
    orc = fr.ForcedOracle(state, cfg, fc.STATS, var_pos_table=variance_position_table(4096, fs["encoder_hidden"]))
    T = g["attn_soft"].shape[1]
    stride = int(g["row_stride"])
    ve = fs["variance"]["variance_embedding"]
    for si in (0, 1):
        pre = f"s{si}_"
        p_t, e_t = fc.targets_of(g)
        p_t = {k: v.copy() for k, v in p_t.items()} if isinstance(p_t, dict) else (None if p_t is None else p_t.copy())
        mel, post, out_lens, (p_ret, e_ret) = orc.forward(g["speakers"], g["ids"], g["txt_lens"], g["mel_lens"], g[pre + "dur"], g["attn_soft"], p_t,
                                                          None if e_t is None else e_t.copy(), soft=si == 0, p_control=float(g["p_control"]),
                                                          max_mel_len=T)
        np.testing.assert_array_equal(out_lens, g[pre + "mel_lens"])
        np.testing.assert_array_equal(orc.trace["pitch_idx"], g[pre + "pitch_idx"])
        np.testing.assert_array_equal(orc.trace["energy_idx"], g[pre + "energy_idx"])
        n_p = out_lens if ve["pitch_feature"] == "frame_level" else g["txt_lens"]
        n_e = out_lens if ve["energy_feature"] == "frame_level" else g["txt_lens"]
        if isinstance(p_ret, dict):
            np.testing.assert_array_equal(p_ret["uv"], g[pre + "p_uv"])
            assert fc.valid_mean_l1(p_ret["f0"], g[pre + "p_f0"], n_p) <= fc.bar(g, pre + "p_f0")
        elif p_ret is not None:
            assert fc.valid_mean_l1(p_ret, g[pre + "p_pitch"], n_p) <= fc.bar(g, pre + "p_pitch")
        else:
            assert pre + "p_f0" not in g and pre + "p_pitch" not in g
        if e_ret is not None:
            assert fc.valid_mean_l1(e_ret, g[pre + "e_tgt"], n_e) <= fc.bar(g, pre + "e_tgt")
        else:
            assert pre + "e_tgt" not in g
        for k, got, rows, st in (("log_d", orc.trace["log_d"], g["txt_lens"], 1), ("pitch_pred", orc.trace["pitch_pred"], n_p, 1),
                                 ("energy_pred", orc.trace["energy_pred"], n_e, 1), ("dec_in", orc.trace["dec_in"], out_lens, stride),
                                 ("mel", mel, out_lens, stride), ("mel_post", post, out_lens, stride)):
            e = fc.valid_mean_l1(got, g[pre + k], rows, st)
            assert e <= fc.bar(g, pre + k), (k, si, e, fc.bar(g, pre + k))


def test_fixtures_cover_what_they_are_for():
    """Sizes, margins and the cases' shapes, as the generator promises them."""
    for name in fc.MODEL_FIXTURES + ["forced_frame2phoneme"]:
        assert os.path.getsize(os.path.join(fc.GOLD, name + ".npz")) < 800 * 1024, name
    for name in fc.MODEL_FIXTURES:
        g = fc.load(name)
        assert float(g["margin"]) >= 1e-3, name
        assert np.array_equal(g["s0_dur"], g["s1_dur"]) and np.array_equal(g["s0_dur"].sum(1), g["mel_lens"])
        assert (g["mel_lens"] >= g["txt_lens"]).all()
    g = fc.load("forced_tiny_b3")
    assert g["attn_soft"].shape == (3, 70, 12) and g["txt_lens"].tolist() == [12, 7, 1] and g["mel_lens"].tolist() == [70, 33, 5]
    assert fc.config_of(g)["models"]["fastspeech2"]["max_seq_len"] < 70
    assert fc.load("forced_tiny_wide_b1")["attn_soft"].shape == (1, 150, 70)
    assert fc.load("forced_full_b2")["attn_soft"].shape == (2, 300, 40) and int(fc.load("forced_full_b2")["row_stride"]) > 1
    p = fc.load("forced_tiny_partial_b3")
    assert "f0" not in p and "energy" in p and float(p["p_control"]) != 1.0 and "s0_p_f0" not in p
    assert "pitch" in fc.load("forced_tiny_nouv_b3") and fc.load("forced_tiny_frame_b3")["s0_pitch_idx"].shape == (3, 70)


def test_frame2phoneme_restated_with_its_in_place_quirk():
    g = fc.load("forced_frame2phoneme")
    dur, lens = g["dur"], g["lens"]
    assert (dur[0, :2] == 0).all() and (dur[5, :4] == 0).all() and dur.max() > 128     # zeros before; a phoneme across numpy's 128-element blocks
    got = fr.get_phoneme_level(g["frames"], lens, dur, dur.shape[1])
    np.testing.assert_array_equal(got.view(np.uint32), g["means"].view(np.uint32))
    np.testing.assert_array_equal(fr.get_phoneme_level(g["uv"], lens, dur, dur.shape[1]).view(np.uint32), g["uv_means"].view(np.uint32))
    # the quirk is there: averaging the untouched frames (out of place) gives other numbers on the rows with leading zeros
    clean = np.zeros_like(got)
    for b in range(dur.shape[0]):
        pos = 0
        for i in range(int(lens[b])):
            d = int(dur[b, i])
            clean[b, i] = np.mean(g["frames"][b, pos:pos + d]) if d else 0.0
            pos += d
    assert not np.array_equal(clean[0], got[0]) and np.array_equal(clean[4], got[4])
    # the input is not modified by the restatement's wrapper
    assert np.array_equal(g["frames"], fc.load("forced_frame2phoneme")["frames"])


def test_header_export_map_and_binding_agree_on_the_new_symbol():
    """The pass has a header and a library of its own (include/e2etts_forced.h, libe2etts_forced.so): header, version script, binding and
    both builds of the library name the same symbols, and the main library's header and exports carry nothing of it."""
    from e2e_tts_amd import _lib, forced
    import __graft_entry__ as g
    header = open(os.path.join(ROOT, "include", "e2etts_forced.h")).read()
    declared = sorted(set(re.findall(r"^E2ETTS_FORCED_API [^;]*?\b(e2etts_[a-z0-9_]+)\s*\(", header, re.M)))
    assert "e2etts_acoustic_forced" in declared and declared == forced.EXPORTED_SYMBOLS
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "forced", "forced.map")).read()
    vmap = re.sub(r"/\*.*?\*/", "", vmap, flags=re.S)
    assert sorted(re.findall(r"^\s*([A-Za-z0-9_]+);", vmap.split("local:")[0], re.M)) == declared
    if g.built_hash() != g.source_hash() or any(g.built_companion_hash(g.FORCED, p) != g.companion_hash(g.FORCED) for p in (g.FORCED["lib"], g.FORCED["test_lib"])):
        g.build()
    for path in (forced.LIB_PATH, forced.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))
        assert exported == declared, (path, exported)
    main = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    main_h = open(os.path.join(ROOT, "include", "e2etts.h")).read()
    assert "forced" not in main and not re.search(r"^E2ETTS_API[^;]*forced", main_h, re.M) and "typedef struct e2etts_forced" not in main_h
    assert "e2etts_acoustic_forced" not in _lib.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(forced.LIB_PATH)       # loads without a GPU
    lib.e2etts_forced_version.restype = lib.e2etts_forced_engine_version.restype = ctypes.c_char_p
    mainlib = ctypes.CDLL(_lib.LIB_PATH)
    mainlib.e2etts_version.restype = ctypes.c_char_p
    assert lib.e2etts_forced_engine_version() == mainlib.e2etts_version()         # one build: the pair works on one engine layout
    assert lib.e2etts_forced_abi_version() == forced.ABI_VERSION == int(re.search(r"#define E2ETTS_FORCED_ABI_VERSION (\d+)", header).group(1))
    assert g.companion_hash(g.FORCED).encode() in lib.e2etts_forced_version()
    # the struct mirror: the header's fields in the header's order, the C compiler's layout (pointers 8-byte aligned after two 32-bit fields)
    body = re.search(r"typedef struct e2etts_forced \{(.*?)\} e2etts_forced;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in forced.CForced._fields_]
    assert ctypes.sizeof(forced.CForced) == 72 and forced.CForced.struct_size.offset == 0 and forced.CForced.durations.offset == 8


@pytest.fixture(scope="module")
def logic(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "forced_logic_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)

    def run(case):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 0, f"sanitizer report or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
        return r.stdout.strip()
    return run


REFUSALS = {   # case -> what the message must name
    "size": r"struct_size = 80",
    "size_zero": r"struct_size = 0",
    "nouv_with_f0": r"pitch_no_uv = 1",
    "uv_with_pitch": r"pitch_no_uv = 0",
    "f0_without_uv": r"uv is NULL",
    "frames_without_durations": r"`durations`, which is NULL",
    "attn_without_T": r"needs T, which is 0",
    "attn_without_mel_lens": r"needs mel_lens, which is NULL",
    "mel_lens_without_attn": r"without attn_soft",
    "mel_len_zero": r"mel_lens\[1\]=0 outside \[1, 10\]",
    "mel_len_past_T": r"mel_lens\[0\]=11 outside \[1, 10\]",
    "T_past_position_table": r"T=4097 exceeds the shipped position table \(4096 rows\)",
    "T_past_var_table": r"T=10 exceeds the variance predictors' position table \(10 rows\)",
    "T_huge": r"T=1048577 is unreasonably large",
    "T_negative": r"T = -3",
    "dur_negative": r"durations\[0, 2\] = -1 is negative",
    "dur_fraction": r"durations\[1, 1\] = 2.5 is not an integer",
    "dur_nan": r"durations\[0, 0\] = -?nan is not finite",
    "dur_inf": r"durations\[1, 3\] = inf is not finite",
    "dur_sum_past_T": r"utterance 0 sum to 11 frames.*T = 10",
    "flag_bad": r"energy_frames = 2",
    "bt_target_without_T": r"needs T, which is 0",
}


def test_every_refusal_names_its_value_under_asan_and_ubsan(logic):
    """forced_check runs before anything is enqueued (engine.hip: acoustic_entry calls it first); here as a program of its own."""
    cases = logic("list").split()
    accepted = {"valid", "valid_hard", "valid_device_arrays", "dur_padding_ignored_in_sum"}
    assert set(cases) == set(REFUSALS) | accepted | {"null"}
    for c in accepted:
        assert logic(c) == "OK", c
    for c, pat in REFUSALS.items():
        out = logic(c)
        assert out.startswith("ERR ") and re.search(pat, out), (c, out)


def test_a_null_struct_is_routed_to_the_ctl_path(logic):
    """Every pointer NULL (whatever the scalars say): forced_is_null, which is what makes acoustic_entry run the predicted pass
    (tests/test_gpu_forced.py: test_null_struct_is_the_ctl_path checks the routing itself, bit for bit)."""
    assert logic("null").split("\n") == ["OK null", "OK non-null"]


def test_f0_targets_restates_the_data_loaders_get_f0():
    """Hz -> (normalised f0 with unvoiced stretches interpolated, uv): equal to the reference method's output on its fixture, both quantizations."""
    from e2e_tts_amd.models import f0_targets
    g = fc.load("forced_get_f0")
    seen_all_uv = seen_edges = False
    for q in ("linear", "log"):
        for i in range(int(g["n"])):
            hz = g[f"hz_{i}"]
            f0, uv = f0_targets(hz, fc.STATS, q)
            assert f0.dtype == g[f"{q}_{i}_f0"].dtype and uv.dtype == np.float32
            np.testing.assert_array_equal(f0, g[f"{q}_{i}_f0"])
            np.testing.assert_array_equal(uv, g[f"{q}_{i}_uv"])
            seen_all_uv |= bool(uv.all())
            seen_edges |= bool(uv[0] and uv[-1] and not uv.all())
            assert np.array_equal(hz, fc.load("forced_get_f0")[f"hz_{i}"])   # the input is not modified
    assert seen_all_uv and seen_edges
    with pytest.raises(ValueError):
        f0_targets(np.zeros((2, 3)), fc.STATS)
