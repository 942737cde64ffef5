"""Fastformer blocks (building_block.block_type "fastformer", reference U/blocks/fastformer.py), everything that needs no GPU: config
flattening, the engine's config validation, synthetic state + packer, and the numpy restatement (tests/fastformer_ref.py) against the
fixtures that tools/make_fastformer_goldens.py wrote from the reference's own run."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from e2e_tts_amd import config as cfgmod, packer, synth_weights as sw
from fastformer_ref import FastformerOracle, fastformer_config

FIXTURES = ("tiny_ff_b3", "tiny_ff_b1", "tiny_ff_long", "full_ff_b2")
FLOATS = ("enc_out", "dec_out", "log_d", "mel", "mel_post")
BAR = 1e-5   # tests/test_oracle_golden.py holds the FFT and Conformer fixtures to this mean-L1
# Arrays for which BAR is replaced by a measured one.  In a row without padding the reference adds -10000 to every logit
# (fastformer.py:223-225,234,253), which rounds it to fp32's grid at 1e4 (2^-10) before the softmax; two fp32 evaluations whose logits
# differ in the last bit land on different sides of such a step now and then, and at full size (192 heads, 1095 frames, 6 + 6 layers) that
# alone puts numpy-fp32 3.6e-5 (enc_out) .. 6.2e-5 (mel_post) from torch-fp32.  That this is rounding and not a different function:
# the same restatement in float64 against the reference run in .double() agrees to 1e-13 (`restate64_*` in the fixture, asserted below).
# The yardstick is the reference's own fp32-vs-float64 distance on the fixture (`f64_*`, 6.2e-5 .. 9.9e-5): the restatement may be
# at most 2 x that far from the reference's fp32 output (the factor covers one more summation order).
MEASURED = {("full_ff_b2", k) for k in ("enc_out", "dec_out", "mel", "mel_post")}


def config_of(name):
    return fastformer_config(cfgmod.tiny_config() if name.startswith("tiny") else cfgmod.default_config())


def bar_for(g, name, k):
    if (name, k) in MEASURED:
        assert float(g["restate64_" + k]) < 1e-12
        return 2.0 * float(g["f64_" + k])
    return BAR


def strided(g, k, x):
    return x[:, ::int(g[k + "_stride"])] if k + "_stride" in g else x


def mean_l1(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def test_dims_from_config_selects_the_block_and_swaps_heads():
    full = fastformer_config(cfgmod.default_config())
    d = cfgmod.dims_from_config(full, cfgmod.DEFAULT_STATS, n_speakers=4)
    assert d.block_type == 2 and d.to_c().block_type == 2
    assert d.ff_heads("enc") == (192, 2) and d.ff_heads("dec") == (192, 2)     # H = 384, encoder_head 2: 192 heads of size 2
    assert (d.ffn_dim, d.ffn_k1, d.ffn_k2) == (1024, 9, 1)
    tiny = fastformer_config(cfgmod.tiny_config(), encoder_head=2, decoder_head=4)
    d = cfgmod.dims_from_config(tiny, cfgmod.DEFAULT_STATS, n_speakers=4)
    assert d.ff_heads("enc") == (32, 2) and d.ff_heads("dec") == (16, 4)
    # the shipped default dict carries the yaml's fastformer section: selecting the block is the one switch
    cfg = cfgmod.default_config()
    cfg["models"]["fastspeech2"]["building_block"]["block_type"] = "fastformer"
    assert cfgmod.dims_from_config(cfg, cfgmod.DEFAULT_STATS, n_speakers=4).block_type == 2
    for bt in ("lstransformer", "reformer"):
        cfg["models"]["fastspeech2"]["building_block"]["block_type"] = bt
        with pytest.raises(NotImplementedError):
            cfgmod.dims_from_config(cfg, cfgmod.DEFAULT_STATS, n_speakers=4)
    with pytest.raises(NotImplementedError):   # head size 3: no instantiation of the pooling kernel
        cfgmod.dims_from_config(fastformer_config(cfgmod.default_config(), encoder_head=3, decoder_head=3), cfgmod.DEFAULT_STATS, n_speakers=4)
    with pytest.raises(ValueError):            # 'same' padding needs an odd kernel
        cfgmod.dims_from_config(fastformer_config(cfgmod.tiny_config(), conv_kernel_size=(4, 1)), cfgmod.DEFAULT_STATS, n_speakers=4)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ffhost") / "host_logic_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "host_logic_test.cc"), "-o", exe], check=True)
    return exe


def test_host_logic_accepts_block_type_2_and_names_what_it_refuses(harness, tmp_path):
    def check(c):
        f = tmp_path / "cfg.bin"
        f.write_bytes(bytes(ctypes.string_at(ctypes.addressof(c), ctypes.sizeof(c))))
        r = subprocess.run([harness, "config", str(f)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip()

    dims = cfgmod.dims_from_config(fastformer_config(cfgmod.tiny_config()), cfgmod.DEFAULT_STATS, n_speakers=4)
    assert check(dims.to_c()).startswith("OK halo=")
    c = dims.to_c()
    c.block_type = 3
    assert check(c) == "ERR block_type must be 0 (FFT block), 1 (Conformer block) or 2 (Fastformer block)"
    c = dims.to_c()
    c.hidden = 68           # a multiple of 4, not of the head size 8
    c.n_head = c.dec_n_head = 8
    assert check(c) == "ERR hidden must be a positive multiple of 4 and of n_head"
    c = dims.to_c()
    c.dec_n_head = 16       # divides 64, but no head size the pooling kernel has
    assert check(c) == "ERR Fastformer: n_head / dec_n_head (the head SIZE of this block) must be 1, 2, 4 or 8"
    c = dims.to_c()
    c.ffn_k1 = 4
    assert check(c) == "ERR FFN kernels must be (odd, 1)"
    c = dims.to_c()
    c.ffn_k2 = 3
    assert check(c) == "ERR FFN kernels must be (odd, 1)"
    c = dims.to_c()
    c.hidden, c.n_head, c.dec_n_head = 2048, 8, 8
    assert check(c) == "ERR Fastformer: hidden must be at most 1024"


def test_synthetic_state_ties_the_logit_layers_and_packs_them_once():
    cfg = fastformer_config(cfgmod.tiny_config(), encoder_head=2, decoder_head=4)
    dims = cfgmod.dims_from_config(cfg, cfgmod.DEFAULT_STATS, n_speakers=4)
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=1234, mode="varied")
    H = dims.hidden
    for side, heads in (("encoder", 32), ("decoder", 16)):
        for w in ("to_q_attn_logits", "to_k_attn_logits"):
            w0 = ac[f"{side}.layer_stack.layers.0.0.fn.{w}.weight"]
            assert w0.shape == (heads, H)
            np.testing.assert_array_equal(ac[f"{side}.layer_stack.layers.1.0.fn.{w}.weight"], w0)
            np.testing.assert_array_equal(ac[f"{side}.layer_stack.layers.1.0.fn.{w}.bias"], ac[f"{side}.layer_stack.layers.0.0.fn.{w}.bias"])
        # logits of order 1 on unit-variance rows: the softmaxes over the sequence are far from uniform
        assert 0.5 < float(ac[f"{side}.layer_stack.layers.0.0.fn.to_q_attn_logits.weight"].std()) * np.sqrt(H) < 4.0
    t = packer.pack_tensors(dims, ac, None)
    np.testing.assert_array_equal(t["enc.ff.wql"], ac["encoder.layer_stack.layers.0.0.fn.to_q_attn_logits.weight"].T)   # [H][heads]
    np.testing.assert_array_equal(t["dec.ff.wkl"], ac["decoder.layer_stack.layers.0.0.fn.to_k_attn_logits.weight"].T)
    assert t["enc.ff.wql"].shape == (H, 32) and t["dec.ff.wql"].shape == (H, 16) and t["dec.ff.bkl"].shape == (16,)
    assert not any(".ff.w" in k and k[:5] not in ("enc.f", "dec.f") for k in t)   # once per side, not per layer
    np.testing.assert_array_equal(t["enc.1.att.wqk"][:H], ac["encoder.layer_stack.layers.1.0.fn.query.weight"])
    np.testing.assert_array_equal(t["enc.1.att.wqk"][H:], ac["encoder.layer_stack.layers.1.0.fn.key.weight"])
    np.testing.assert_array_equal(t["dec.0.att.bqk"][H:], ac["decoder.layer_stack.layers.0.0.fn.key.bias"])
    w1 = ac["decoder.layer_stack.layers.1.1.fn.w_1.weight"]                                  # [F, H, k] -> tap-major [F, k * H]
    np.testing.assert_array_equal(t["dec.1.ffn.w1"].reshape(w1.shape[0], w1.shape[2], H), w1.transpose(0, 2, 1))
    assert "dec.1.ffn.w1.x3" in t and "dec.0.att.wqk.x3" in t and "enc.0.att.wqk.x3" not in t   # split precision: decoder GEMMs only
    # blob round trip: every tensor back bit for bit
    blob = packer.build_blob(t)
    import struct
    n = struct.unpack_from("<I", blob, 12)[0]
    assert n == len(t)
    for i, (name, arr) in enumerate(t.items()):
        raw, off, numel = struct.unpack_from("<64sQQ", blob, 32 + 80 * i)
        assert raw.rstrip(b"\0").decode() == name and numel == arr.size
        np.testing.assert_array_equal(blob[off:off + 4 * numel].view(np.float32), arr.reshape(-1))
    # a checkpoint whose later layer carries logit weights of its own is not one the reference's module wrote
    bad = dict(ac)
    bad["encoder.layer_stack.layers.1.0.fn.to_q_attn_logits.weight"] = bad["encoder.layer_stack.layers.1.0.fn.to_q_attn_logits.weight"] + np.float32(1e-3)
    with pytest.raises(ValueError, match="ties these projections"):
        packer.pack_tensors(dims, bad, None)
    missing = {k: v for k, v in ac.items() if k != "decoder.layer_stack.layers.1.0.fn.transform.bias"}
    with pytest.raises(KeyError):
        packer.pack_tensors(dims, missing, None)


# sha256 over (name, dtype, shape, bytes) of make_acoustic_state's tensors, recorded on the commit before the fastformer manifest was added:
# every existing fixture regenerates its weights from seeds, so the streams of the other two blocks must not move
PARENT_DIGESTS = {
    ("tiny", "transformer"): ("3e642db1cb4be436740c45e877ea263beaf1d1f96587ac5a0b21b941d45913f0", "9b907a6224dd7d5d1a40a9656e6451c4ed7c5aa98574ead677b210b55f4e1f02"),
    ("tiny", "conformer"): ("77297eef61ccc254b9b5776ff2edb9e8677ade88f50e8fd1a59323af2868db19", "9935d77052ddf278a00567d0feb25d823cf3bee95fca358ce44753a237132bb9"),
    ("default", "transformer"): ("c58de695d60121afcac11fb27c3c599ef74e85989d5db24e9c24913d9d32e73b", "810a3283a5b944353af96c2f4312735a0bc6f88a7e0a55f4d9913be8d31828b0"),
    ("default", "conformer"): ("67040f8013abbb1e9c158fc311d1d685865c3e8e0519c53845b4a63d7de14598", "f5e2818d0d229b03000f174514c3955fa98c2fd4a26d04030fd848be35ef1fc6"),
}


@pytest.mark.parametrize("size,bt", sorted(PARENT_DIGESTS))
def test_states_of_the_other_blocks_are_what_they_were(size, bt):
    def digest(cfg, **kw):
        h = hashlib.sha256()
        for k, v in sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, **kw).items():
            h.update(k.encode() + b"\0" + str(v.dtype).encode() + str(v.shape).encode())
            h.update(v.tobytes())
        return h.hexdigest()

    cfg = getattr(cfgmod, size + "_config")()
    cfg["models"]["fastspeech2"]["building_block"]["block_type"] = bt
    assert (digest(cfg, seed=1234, mode="varied"), digest(cfg, seed=7, mode="fixed")) == PARENT_DIGESTS[(size, bt)]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference_fixture(name):
    """tests/fastformer_ref.py (numpy fp32) against the reference's own run (torch fp32, CPU): discrete outputs exact, float arrays mean-L1
    < 1e-5 -- or, for the arrays listed in MEASURED, within twice the reference's own fp32-vs-float64 distance.

    Measured (numpy fp32 vs the fixture; in brackets the fixture's f64 yardstick):
      tiny_ff_b3    enc_out 3.8e-7 (2.8e-5)  dec_out 8.5e-7 (4.2e-5)  log_d 2.4e-7 (1.2e-5)  mel 9.5e-7 (4.2e-5)  mel_post 1.0e-6 (4.3e-5)
      tiny_ff_b1    enc_out 5.2e-7 (2.3e-4)  dec_out 6.1e-6 (3.2e-4)  log_d 3.1e-7 (9.5e-5)  mel 6.5e-6 (3.3e-4)  mel_post 6.6e-6 (3.4e-4)
      tiny_ff_long  enc_out 1.3e-6 (3.3e-5)  dec_out 4.3e-6 (4.8e-5)  log_d 5.5e-7 (1.3e-5)  mel 4.7e-6 (4.9e-5)  mel_post 4.8e-6 (5.0e-5)
      full_ff_b2    enc_out 3.6e-5 (6.2e-5)  dec_out 5.8e-5 (9.2e-5)  log_d 8.9e-6 (1.5e-5)  mel 6.1e-5 (9.7e-5)  mel_post 6.2e-5 (9.9e-5)"""
    g = load_golden(name)
    cfg = config_of(name)
    ac = sw.make_acoustic_state(cfg, cfgmod.DEFAULT_STATS, 4, seed=int(g["weight_seeds"][0]), mode=str(g["mode"]))
    o = FastformerOracle(ac, cfg, cfgmod.DEFAULT_STATS)
    d, p, e = (float(x) for x in g["controls"])
    (mel, mel_post, dur), mel_lens = o.inference(np.array([int(g["speaker"])], np.int64), g["ids"], g["lens"], d, p, e)
    np.testing.assert_array_equal(dur, g["dur"])
    np.testing.assert_array_equal(mel_lens, g["mel_lens"])
    np.testing.assert_array_equal(o.trace["pitch_idx"], g["pitch_idx"])
    np.testing.assert_array_equal(o.trace["energy_idx"], g["energy_idx"])
    got = dict(enc_out=o.trace["enc_out"], dec_out=o.trace["dec_out"], log_d=o.trace["log_d"], mel=mel, mel_post=mel_post)
    for k in FLOATS:
        err = mean_l1(strided(g, k, got[k]), g[k])
        print(f"{name} {k}: mean-L1 {err:.3e} (bar {bar_for(g, name, k):.3e}; reference fp32 vs float64 {float(g['f64_' + k]):.3e})")
        assert err < bar_for(g, name, k), (name, k, err)
    # the same function: float64 restatement vs the reference in .double(), recorded by the golden tool
    for k in FLOATS:
        assert float(g["restate64_" + k]) < 1e-12, (k, float(g["restate64_" + k]))


def test_fixtures_fit_the_repository_limit():
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20


def test_both_libraries_carry_the_fastformer_kernels_and_no_new_export():
    """build() compiles csrc/fastformer.hip into the product and the test library; the block needs no entry point of its own."""
    import __graft_entry__ as ge
    from e2e_tts_amd import _lib
    for path in (ge.LIB, ge.TEST_LIB):
        blob = open(path, "rb").read()
        assert b"ff_pool_partial_kernel" in blob and b"ff_pool_merge_kernel" in blob and b"ff_scale_kernel" in blob, path
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert not any("ff_" in s or "fastformer" in s for s in syms), sorted(syms)
        assert set(_lib.EXPORTED_SYMBOLS) <= syms
