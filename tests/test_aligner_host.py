"""Forced alignment, the parts that need no GPU: the numpy restatement (tests/aligner_ref.py) against the reference's fixtures
(tools/make_aligner_goldens.py), the beta-binomial prior, the aligner's weight blob, and the companion library's C ABI -- its exports and
its argument validation, which runs before a device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import aligner_ref as ar
from aligner_cases import FORWARD_FIXTURES, MAX_BAR, MEAN_BAR, fixture_inputs
from e2e_tts_amd import aligner as al, config as cfgmod, packer, synth_weights as sw

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if g.built_align_hash() != g.align_hash() or g.built_align_hash(g.AL_TEST_LIB) != g.align_hash():
        g.build()
    return al.load_library()


@pytest.mark.parametrize("name", FORWARD_FIXTURES)
def test_restatement_mas_equals_the_reference_on_its_log_map(name):
    g = load_golden(name)
    with np.errstate(divide="ignore"):
        loga = np.log(g["attn"])
    for search in (ar.mas_loops, ar.mas_rows):
        if search is ar.mas_loops and g["attn"].size > 12000:
            continue   # the plain loops on the small maps, the row form on all
        hard = ar.b_mas(loga, g["txt_lens"], g["mel_lens"], log_map=True, search=search)
        assert np.array_equal(hard, g["attn_hard"].astype(np.float32))
        assert np.array_equal(hard.sum(1), g["dur"])
    ok = g["mel_lens"] >= g["txt_lens"]
    assert np.array_equal(g["dur"].sum(1)[ok], g["mel_lens"][ok].astype(np.float32))


@pytest.mark.parametrize("tag", ["eq", "short", "plain"])
def test_restatement_mas_on_the_degenerate_maps(tag):
    g = load_golden("aligner_mas_only")
    attn, il, ol = g[f"{tag}_attn"], g[f"{tag}_in_lens"], g[f"{tag}_out_lens"]
    for search in (ar.mas_loops, ar.mas_rows):
        hard = ar.b_mas(attn, il, ol, search=search)
        assert np.array_equal(hard, g[f"{tag}_attn_hard"].astype(np.float32))
    if tag == "eq":
        assert all(np.array_equal(g["eq_dur"][b, :n], np.ones(n, np.float32)) for b, n in enumerate(il))
    if tag == "short":   # the path never reaches column 0: the closing assignment puts a second 1 into row 0
        assert all(g["short_attn_hard"][b, 0].sum() == 2 and g["short_attn_hard"][b, 0, 0] == 1 for b in range(len(il)))


@pytest.mark.parametrize("name", FORWARD_FIXTURES)
def test_restatement_fp32_forward_within_the_bars_of_the_float64_fixture(name):
    g = load_golden(name)
    state, keys, spk, prior = fixture_inputs(g)
    P = ar.submodule_state(state)
    cases = [("", g["txt_lens"])]
    if "nomask_attn" in g:
        cases.append(("nomask_", None))
    for pre, lens in cases:
        attn, logprob = ar.forward(P, g["mel"].transpose(0, 2, 1), keys.transpose(0, 2, 1), float(g["temperature"]), lens, prior, spk, dtype=np.float32)
        cols = g["txt_lens"] if lens is not None else np.full(len(g["txt_lens"]), keys.shape[1])
        ea = ar.valid_stats(attn, g[pre + "attn64"], cols, g["mel_lens"])
        el = ar.valid_stats(logprob, g[pre + "attn_logprob64"], cols, g["mel_lens"], full_columns=True)
        ra, rl = g[pre + "ref_err_attn"], g[pre + "ref_err_logprob"]
        print(f"{name} {pre}: attn mean {ea[0]:.3e} max {ea[1]:.3e} (reference {ra[0]:.3e} / {ra[1]:.3e}); logprob mean {el[0]:.3e} max {el[1]:.3e} "
              f"(reference {rl[0]:.3e} / {rl[1]:.3e})")
        assert ea[0] <= MEAN_BAR * ra[0] and ea[1] <= MAX_BAR * ra[1]
        assert el[0] <= MEAN_BAR * rl[0] and el[1] <= MAX_BAR * rl[1]
        if lens is not None:
            for b, n in enumerate(lens):
                assert not attn[b, :, n:].any() and np.isfinite(logprob[b]).all()


def test_prior_equals_the_fixtures():
    for name in ("aligner_tiny_b3", "aligner_tiny_wide_b1"):
        g = load_golden(name)
        T, L = g["mel"].shape[1], g["ids"].shape[1]
        assert np.array_equal(al.batch_prior(g["txt_lens"], g["mel_lens"], T, L), g["prior"])
        assert np.array_equal(ar.pad_prior([ar.beta_binomial_prior(int(p), int(m)) for p, m in zip(g["txt_lens"], g["mel_lens"])], T, L), g["prior"])
    p = al.beta_binomial_prior_distribution(7, 33, 1.0)
    # betabinom(P, a, b) lives on 0 .. P and the reference evaluates it on 0 .. P - 1: the rows do not sum to 1.  Frame 1 of 33 on phoneme 0:
    # B(1, 33 + 7) / B(1, 33) = 33 / 40
    assert p.shape == (33, 7) and p.dtype == np.float64 and (p.sum(1) < 1.0).all() and abs(p[0, 0] - 33.0 / 40.0) < 1e-12
    assert p[0].argmax() == 0 and p[-1].argmax() == 6   # (the last row's mass peaks at P, outside what is evaluated)


def read_blob(blob):
    import struct
    magic, ver, n, data_off, total = struct.unpack("<8sIIQQ", blob[:32].tobytes())
    assert magic == packer.MAGIC and total == blob.size
    out = {}
    for i in range(n):
        raw, off, numel = struct.unpack("<64sQQ", blob[32 + 80 * i:112 + 80 * i].tobytes())
        out[raw.rstrip(b"\0").decode()] = blob[off:off + 4 * numel].view(np.float32)
    return out


def test_pack_aligner_round_trips_and_leaves_pack_alone():
    cfg = cfgmod.tiny_config()
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=1234, mode="varied")
    dims = cfgmod.dims_from_config(cfg, cfgmod.DEFAULT_STATS, 4)
    H, M = 64, 80
    assert packer.aligner_dims(state) == (M, M, H)
    t = read_blob(packer.pack_aligner(state))
    pre = packer.ALIGNER_PREFIX
    assert sorted(t) == sorted(["aln.key.0.w", "aln.key.0.b", "aln.key.2.w", "aln.key.2.b", "aln.query.0.w", "aln.query.0.b", "aln.query.2.w", "aln.query.2.b",
                                "aln.query.4.w", "aln.query.4.b", "aln.key_spk.w", "aln.query_spk.w"])
    for name, key in (("aln.key.0", "key_proj.0"), ("aln.key.2", "key_proj.2"), ("aln.query.0", "query_proj.0"), ("aln.query.2", "query_proj.2"),
                      ("aln.query.4", "query_proj.4")):
        w = state[f"{pre}{key}.conv.weight"]
        back = t[name + ".w"].reshape(w.shape[0], w.shape[2], w.shape[1]).transpose(0, 2, 1)   # tap-major rows -> [Cout, Cin, K]
        assert np.array_equal(back, w) and np.array_equal(t[name + ".b"], state[f"{pre}{key}.conv.bias"])
    assert np.array_equal(t["aln.key_spk.w"].reshape(H, H), state[pre + "key_spk_proj.linear.weight"])
    assert np.array_equal(t["aln.query_spk.w"].reshape(M, H), state[pre + "query_spk_proj.linear.weight"])
    # the submodule's own state dict (prefix "") packs to the same bytes
    assert np.array_equal(packer.pack_aligner(ar.submodule_state(state), ""), packer.pack_aligner(state))
    assert not any(k.startswith("aln.") for k in packer.pack_tensors(dims, state, None))
    with pytest.raises(KeyError):
        packer.pack_aligner({k: v for k, v in state.items() if not k.startswith(pre)})


@pytest.mark.slow
def test_pack_of_the_default_config_never_sees_the_aligner():
    """packer.pack for the default config: the blob of a checkpoint equals, byte for byte, the blob built from the same state without its
    aligner tensors and the blob of the same state with other aligner weights -- nothing of the aligner enters it, so it is what it was before
    pack_aligner existed (tests/test_fastformer_host.py pins such blobs by hash)."""
    cfg = cfgmod.default_config()
    state = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=11, mode="varied")
    dims = cfgmod.dims_from_config(cfg, cfgmod.DEFAULT_STATS, 4)
    pre = packer.ALIGNER_PREFIX
    main = packer.pack(dims, state, None)
    assert np.array_equal(main, packer.pack(dims, {k: v for k, v in state.items() if not k.startswith(pre)}, None))
    other = {k: (v * np.float32(3) if k.startswith(pre) else v) for k, v in state.items()}
    assert np.array_equal(main, packer.pack(dims, other, None))
    assert packer.aligner_dims(state) == (80, 80, 384)


def test_library_loads_without_a_gpu_and_exports_its_header(lib):
    header = open(os.path.join(ROOT, "include", "e2etts_align.h")).read()
    hooks_block = re.search(r"#ifdef E2EALIGN_TEST_HOOKS\n(.*?)#endif", header, re.S).group(1)
    hook_syms = sorted(set(re.findall(r"\b(e2ealign_[a-z0-9_]+)\s*\(", hooks_block)))
    declared_all = sorted(set(re.findall(r"^E2EALIGN_API [^;]*?\b(e2ealign_[a-z0-9_]+)\s*\(", header, re.M)))
    declared = [d for d in declared_all if d not in hook_syms]
    assert hook_syms == sorted(al.TEST_HOOK_SYMBOLS) and declared == sorted(al.EXPORTED_SYMBOLS)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if not s.startswith(("_init", "_fini", "__")))

    assert exported(al.LIB_PATH) == declared, sorted(set(exported(al.LIB_PATH)) ^ set(declared))       # the product library: no test hook
    assert exported(al.TEST_LIB_PATH) == sorted(declared + hook_syms)
    plain = C.CDLL(al.LIB_PATH)                                                                       # loads without a GPU
    for sym in declared:
        assert hasattr(plain, sym), sym
    assert lib.e2ealign_abi_version() == al.ABI_VERSION == int(re.search(r"#define E2EALIGN_ABI_VERSION (\d+)", header).group(1))
    for name, val in (("E2EALIGN_MAX_ATT", al.MAX_ATT), ("E2EALIGN_MAX_L", al.MAX_L), ("E2EALIGN_MAX_B", al.MAX_B), ("E2EALIGN_LOG_MAP", al.LOG_MAP)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    import __graft_entry__ as g
    assert g.align_hash() in lib.e2ealign_version().decode()
    # the main library's symbols are untouched by the companion: nothing of it is exported there
    from e2e_tts_amd import _lib
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "e2ealign_" not in syms


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal below happens on the host, before the handle opens a device: the test runs without a GPU, and the handle stays usable
    (device_bytes stays 0: nothing was allocated)."""
    P = C.c_void_p
    h = P()
    for bad in ((0, 80, 80, 62), (0, 0, 80, 64), (0, 80, 129, 64), (-1, 80, 80, 64), (0, 82, 80, 64)):
        assert lib.e2ealign_create(bad[0], bad[1], bad[2], bad[3], 5e-4, C.byref(h)) == al.E_INVAL and not h.value
        assert b"e2ealign_create" in lib.e2ealign_last_error(None)
    assert lib.e2ealign_create(0, 80, 80, 64, 5e-4, C.byref(h)) == al.E_OK and h.value
    B, T, L = 2, 6, 5
    amap = np.full((B, T, L), 0.2, np.float32)
    hard, dur = np.zeros((B, T, L), np.float32), np.zeros((B, L), np.float32)
    ok_in, ok_out = np.array([5, 3], np.int64), np.array([6, 4], np.int64)

    def mas(m, il, ol, B=B, T=T, L=L, flags=0):
        return lib.e2ealign_mas(h, None if m is None else m.ctypes.data, flags, il.ctypes.data, ol.ctypes.data, B, T, L, hard.ctypes.data, dur.ctypes.data)

    assert mas(amap, ok_in, ok_out, B=-1) == al.E_INVAL
    assert mas(amap, ok_in, ok_out, T=0) == al.E_INVAL
    assert mas(amap, ok_in, ok_out, L=-3) == al.E_INVAL
    assert mas(amap, ok_in, ok_out, L=al.MAX_L + 1) == al.E_INVAL
    assert mas(amap, np.array([6, 3], np.int64), ok_out) == al.E_INVAL and b"in_lens[0] = 6" in lib.e2ealign_last_error(h)     # in_len > L
    assert mas(amap, ok_in, np.array([6, 7], np.int64)) == al.E_INVAL and b"out_lens[1] = 7" in lib.e2ealign_last_error(h)    # out_len > T
    assert mas(amap, np.array([5, 0], np.int64), ok_out) == al.E_INVAL                                                        # lens < 1
    assert mas(amap, ok_in, np.array([-2, 4], np.int64)) == al.E_INVAL
    assert mas(amap, ok_in, ok_out, flags=8) == al.E_INVAL
    assert mas(None, ok_in, ok_out) == al.E_INVAL and b"resident" in lib.e2ealign_last_error(h)                               # NULL map, nothing resident
    # forward / align: sizes and lengths are checked first, then the missing weights are a matter of call order
    mel, keys = np.zeros((B, T, 80), np.float32), np.zeros((B, L, 64), np.float32)
    fw = lambda B_, T_, L_: lib.e2ealign_forward(h, mel.ctypes.data, keys.ctypes.data, None, None, None, B_, T_, L_, None, None)  # noqa: E731
    assert fw(0, T, L) == al.E_INVAL and fw(B, -1, L) == al.E_INVAL and fw(B, T, 0) == al.E_INVAL
    assert fw(B, T, L) == al.E_STATE
    # a blob with a tensor missing, a tensor of another size, a truncated blob
    state = sw.make_aligner_state(64, 80, seed=5)
    tensors = packer.pack_aligner_tensors(state)
    for drop in ("aln.query.4.b", "aln.key_spk.w"):
        blob = packer.build_blob({k: v for k, v in tensors.items() if k != drop})
        assert lib.e2ealign_load_weights(h, blob.ctypes.data, blob.size) == al.E_INVAL and drop.encode() in lib.e2ealign_last_error(h)
    wrong = packer.pack_aligner(sw.make_aligner_state(32, 80, seed=5))
    assert lib.e2ealign_load_weights(h, wrong.ctypes.data, wrong.size) == al.E_INVAL and b"elements" in lib.e2ealign_last_error(h)
    good = packer.build_blob(tensors)
    assert lib.e2ealign_load_weights(h, good.ctypes.data, good.size - 256) == al.E_INVAL
    assert lib.e2ealign_load_weights(h, None, 0) == al.E_INVAL
    assert lib.e2ealign_device_bytes(h) == 0
    # still usable: the same refusals, the same messages
    assert mas(None, ok_in, ok_out) == al.E_INVAL and b"resident" in lib.e2ealign_last_error(h)
    assert lib.e2ealign_sync(h) == al.E_OK
    lib.e2ealign_destroy(h)
    with pytest.raises(ValueError):
        al.Aligner(80, 500, 64, 5e-4)
