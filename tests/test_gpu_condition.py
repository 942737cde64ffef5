"""libe2etts_condition.so on the GPU, bit for bit against the plain-integer definition (tests/condition_ref.py) and against what audioop
gave (tests/golden/condition_cases.npz): silence ranges, kept spans, sums of squares, the gained PCM and its fp32 form, the downmix; host
and device inputs, guard bands around every output, poisoned workspaces, the capacity overflow.  No tolerances."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from conftest import ROOT
import condition_cases as cc
import condition_ref as cr
from e2e_tts_amd import condition as cd

pytestmark = pytest.mark.gpu

TRIMS = (("none", None), ("reference", "reference"), ("both", "both"))
_C, _CASES, _REF = {}, {}, {}


def conditioner(rate):
    if rate not in _C:
        _C[rate] = cd.Conditioner(rate)
        assert _C[rate].tile_starts == 512   # what the edge rows of condition_cases are laid out around
    return _C[rate]


def case(name):
    """(rate, channels, raw rows, mono rows), built once"""
    if not _CASES:
        for k, v in cc.cases().items():
            _CASES[k] = (v["rate"], v["channels"], v["rows"], cc.mono_rows(v))
    return _CASES[name]


def ref(name, b, trim, loud):
    key = (name, b, trim, loud)
    if key not in _REF:
        rate, _, _, mono = case(name)
        _REF[key] = cr.normalize(mono[b], rate, trim, loud)
    return _REF[key]


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(ROOT, "tests", "golden", "condition_cases.npz"))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def stereo_batch(rows):
    lens = np.array([len(r) for r in rows], np.int64)
    out = np.zeros((len(rows), int(lens.max()), 2), np.int16)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, lens


NAMES = ["r8000", "r22050", "r44100s"]


@pytest.mark.parametrize("name", NAMES)
def test_analysis_equals_the_definition_and_audioop(name, golden):
    rate, _, _, mono = case(name)
    c = conditioner(rate)
    x, lens = cr.batch(mono)
    assert max(cr.len_ms(int(n), rate) for n in lens) - cc.W + 1 > 2 * c.tile_starts      # the longest row's starts span at least three tiles
    assert any(cr.pos(cr.len_ms(int(n), rate), rate) > n for n in lens)                   # a row whose pos(len_ms) overhangs N
    for gname, trim in TRIMS:
        a = c.analyze(x, lens, trim)
        for b in range(len(mono)):
            key = f"{name}/{b}"
            r = ref(name, b, trim, None)
            assert a["ranges"][b] == r["ranges"] == golden[f"{key}/ranges"].tolist(), (key, gname)
            assert int(a["len_ms"][b]) == int(golden[f"{key}/len_ms"]) and int(a["n_ranges"][b]) == len(r["ranges"])
            assert [int(a["s_ms"][b]), int(a["e_ms"][b]), int(a["n_out"][b])] == [r["s_ms"], r["e_ms"], r["n_out"]] == golden[f"{key}/{gname}/span"].tolist(), (key, gname)
            assert int(a["sumsq"][b]) == r["sumsq"] == int(golden[f"{key}/{gname}/sumsq"]), (key, gname)
    assert c.detect_silence(x, lens) == [ref(name, b, None, None)["ranges"] for b in range(len(mono))]
    want = [cd.dbfs_of(cr.rms(m)) for m in mono]
    assert c.dbfs(x, lens).tolist() == want


@pytest.mark.parametrize("name", NAMES)
def test_normalize_every_sample(name, golden):
    rate, _, _, mono = case(name)
    c = conditioner(rate)
    x, lens = cr.batch(mono)
    for gname, trim in TRIMS:
        for loud in (None, cc.TARGET_DBFS):
            r = c.normalize(x, lens, trim=trim, loudness_dBFS=loud, want=("pcm", "wav"))
            W = r["width"]
            assert r["pcm"].shape == r["wav"].shape == (len(mono), W) and W == int(r["n_out"].max())
            for b in range(len(mono)):
                e = ref(name, b, trim, loud)
                n = e["n_out"]
                assert int(r["n_out"][b]) == n and r["gain"][b] == e["gain"]
                assert np.array_equal(r["pcm"][b, :n], e["pcm"]), (name, b, gname, loud)
                assert not r["pcm"][b, n:].any() and not r["wav"][b, n:].any()
                assert np.array_equal(r["wav"][b], r["pcm"][b].astype(np.float32) / np.float32(32768.0))
                gk = f"{name}/{b}/{gname}/" + ("mul_sha" if loud is not None else "mul1_sha")
                assert np.array_equal(sha(r["pcm"][b, :n]), golden[gk]), gk
                if loud is not None:
                    assert r["gain"][b] == float(golden[f"{name}/{b}/{gname}/gain"])


def test_downmix(golden):
    import torch
    rate, channels, rows, mono = case("r44100s")
    assert channels == 2
    c = conditioner(rate)
    st, lens = stereo_batch(rows)
    B, n = st.shape[:2]
    got = c.downmix(st)
    for b in range(B):
        assert np.array_equal(got[b, :lens[b]], mono[b]) and np.array_equal(sha(got[b, :lens[b]]), golden[f"r44100s/{b}/tomono_sha"])
        assert not got[b, lens[b]:].any()
    assert np.array_equal(c.downmix(torch.from_numpy(st).cuda()), got)                               # a device input
    assert np.array_equal(c.downmix(st.reshape(B, 2 * n)), got)                                      # [B, 2 n] interleaved
    wide = np.zeros((B, 2 * n + 6), np.int16)                                                        # rows off the 16-byte grid: the 2-byte loads
    wide[:, 2:2 * n + 2] = st.reshape(B, 2 * n)
    assert np.array_equal(c.downmix(wide[:, 2:2 * n + 2]), got)
    assert np.array_equal(c.downmix(torch.from_numpy(wide).cuda()[:, 2:2 * n + 2]), got)
    odd = st[:, :n - 3]                                                                              # n not a multiple of 4
    assert np.array_equal(c.downmix(np.ascontiguousarray(odd)), got[:, :n - 3])
    # the chain on the resident downmix: channels = 2 equals the mono rows
    r = c.normalize(st, lens, channels=2, trim="reference", loudness_dBFS=cc.TARGET_DBFS)
    for b in range(B):
        e = ref("r44100s", b, "reference", cc.TARGET_DBFS)
        assert int(r["n_out"][b]) == e["n_out"] and np.array_equal(r["pcm"][b, :e["n_out"]], e["pcm"])


def test_host_and_device_inputs_give_the_same_bits():
    import torch
    rate, _, _, mono = case("r22050")
    c = conditioner(rate)
    x, lens = cr.batch(mono)
    B, n = x.shape
    base = c.normalize(x, lens, trim="both", loudness_dBFS=cc.TARGET_DBFS, want=("pcm", "wav"))
    big = np.zeros((B, n + 11), np.int16)
    for off in (0, 3):                                                                               # rows on and off the 16-byte grid
        big[:] = 0
        big[:, off:off + n] = x
        for src in (big[:, off:off + n], torch.from_numpy(big).cuda()[:, off:off + n]):
            r = c.normalize(src, lens, trim="both", loudness_dBFS=cc.TARGET_DBFS, want=("pcm", "wav"))
            assert np.array_equal(r["pcm"], base["pcm"]) and np.array_equal(r["wav"], base["wav"]) and r["ranges"] == base["ranges"]
            assert np.array_equal(r["n_out"], base["n_out"]) and np.array_equal(r["gain"], base["gain"])
    # a row equals a B = 1 call on that row
    for b in range(B):
        r = c.normalize(x[b:b + 1, :max(1, int(lens[b]))], lens[b:b + 1], trim="both", loudness_dBFS=cc.TARGET_DBFS)
        nb = int(base["n_out"][b])
        assert int(r["n_out"][0]) == nb and np.array_equal(r["pcm"][0, :nb], base["pcm"][b, :nb])
    # the resident outputs: what the mel library and the resampler read where it lies
    c.normalize(x, lens, trim="both", loudness_dBFS=cc.TARGET_DBFS, want=("pcm", "wav"))
    pcm_dev, wav_dev = c.resident()
    W = base["width"]
    assert pcm_dev.shape == (B, W) and pcm_dev.stride(0) % 8 == 0 and pcm_dev.stride(0) >= W
    from e2e_tts_amd import resample as rs
    copy = rs.Resampler(1, 1, taps=np.ones(1, np.float32))                                           # the single tap 1.0: an exact copy
    assert np.array_equal(copy.forward(wav_dev, want=("wav",))["wav"], base["wav"])
    assert np.array_equal(copy.forward(pcm_dev, want=("pcm",))["pcm"], base["pcm"])
    copy.close()


def test_guard_bands_around_every_output():
    import torch
    rate, _, _, mono = case("r8000")
    c = conditioner(rate)
    x, lens = cr.batch(mono)
    B, n = x.shape
    base = c.normalize(x, lens, trim="reference", loudness_dBFS=cc.TARGET_DBFS, want=("pcm", "wav"))
    W = base["width"]
    c.analyze(x, lens, "reference")
    pad = 5
    for dev in (False, True):
        pcm = np.full((B + 1, W + pad), 0x5555, np.int16)
        wav = np.full((B + 1, W + pad), 7.0, np.float32)
        if dev:
            pcm, wav = torch.from_numpy(pcm).cuda(), torch.from_numpy(wav).cuda()
        c.apply(base["gain"], out_pcm=pcm, out_wav=wav, out_stride=W + pad)
        if dev:
            pcm, wav = pcm.cpu().numpy(), wav.cpu().numpy()
        assert np.array_equal(pcm[:B, :W], base["pcm"]) and np.array_equal(wav[:B, :W], base["wav"])
        assert (pcm[:B, W:] == 0x5555).all() and (pcm[B] == 0x5555).all() and (wav[:B, W:] == 7.0).all() and (wav[B] == 7.0).all()
    with pytest.raises(ValueError):
        c.apply(base["gain"], out_pcm=np.zeros((B, W + pad), np.int16), out_stride=W - 1)
    # the records, the ranges and the downmix, at the C level
    lib, cap = c.lib, 6
    rows = np.zeros(B + 1, cd.ROW_DTYPE)
    rows["len_ms"] = -7
    ranges = np.full((B + 1, cap, 2), -7, np.int32)
    assert lib.e2econd_analyze(c._h, x.ctypes.data, n, lens.ctypes.data, B, n, cd.TRIM_REFERENCE, cap, rows.ctypes.data, ranges.ctypes.data) == cd.E_OK
    assert rows["len_ms"][B] == -7 and (ranges[B] == -7).all()
    for b in range(B):
        e = ref("r8000", b, "reference", None)
        k = len(e["ranges"])
        assert ranges[b, :k].tolist() == e["ranges"] and not ranges[b, k:].any() and int(rows["n_ranges"][b]) == k
    rows_d, ranges_d = torch.zeros(B * 32 + 32, dtype=torch.uint8, device="cuda"), torch.full((B + 1, cap, 2), -7, dtype=torch.int32, device="cuda")
    rows_d[B * 32:] = 0x55
    assert lib.e2econd_analyze(c._h, x.ctypes.data, n, lens.ctypes.data, B, n, cd.TRIM_REFERENCE, cap, rows_d.data_ptr(), ranges_d.data_ptr()) == cd.E_OK
    assert np.array_equal(rows_d.cpu().numpy()[:B * 32].view(cd.ROW_DTYPE), rows[:B]) and (rows_d.cpu().numpy()[B * 32:] == 0x55).all()
    assert np.array_equal(ranges_d.cpu().numpy(), ranges)
    st = np.random.Generator(np.random.PCG64(2)).integers(-32768, 32768, (2, 37, 2)).astype(np.int16)
    mono_out = np.full((3, 37 + pad), 0x5555, np.int16)
    assert lib.e2econd_downmix(c._h, st.ctypes.data, 74, 2, 37, mono_out.ctypes.data, 37 + pad) == cd.E_OK
    assert np.array_equal(mono_out[:2, :37], np.stack([cr.downmix(s) for s in st])) and (mono_out[:2, 37:] == 0x5555).all() and (mono_out[2] == 0x5555).all()


def test_poisoned_workspaces_and_capacity_overflow():
    rate, _, _, mono = case("r22050")
    c = conditioner(rate)
    x, lens = cr.batch(mono)
    B, n = x.shape
    base = c.normalize(x, lens, trim="reference", loudness_dBFS=cc.TARGET_DBFS, want=("pcm", "wav"))
    c.poison_workspace()
    with pytest.raises(RuntimeError):
        c.resident()
    with pytest.raises(RuntimeError):                                                                # E2ECOND_ESTATE: the analysis is gone
        c.apply(base["gain"])
    r = c.normalize(x, lens, trim="reference", loudness_dBFS=cc.TARGET_DBFS, want=("pcm", "wav"))
    assert np.array_equal(r["pcm"], base["pcm"]) and np.array_equal(r["wav"], base["wav"]) and r["ranges"] == base["ranges"]
    # the edge row has 5 ranges: cap 2 reports the true count, lists the first two, and refuses
    assert len(base["ranges"][1]) == 5
    with pytest.raises(ValueError, match="row 1 has 5 silence ranges, cap is 2"):
        c.analyze(x, lens, "reference", cap=2)
    rows = np.zeros(B, cd.ROW_DTYPE)
    ranges = np.full((B + 1, 2, 2), -7, np.int32)
    assert c.lib.e2econd_analyze(c._h, x.ctypes.data, n, lens.ctypes.data, B, n, cd.TRIM_REFERENCE, 2, rows.ctypes.data, ranges.ctypes.data) == cd.E_INVAL
    assert rows["n_ranges"].tolist() == [len(v) for v in base["ranges"]] and ranges[1].tolist() == base["ranges"][1][:2] and (ranges[B] == -7).all()
    assert [int(v) for v in rows["n_out"]] == [int(v) for v in base["n_out"]]                        # the span does not depend on cap
    g = np.ones(B)
    w = C.c_longlong(-7)
    assert c.lib.e2econd_apply(c._h, g.ctypes.data, cd.WANT_PCM, None, None, 0, C.byref(w)) == cd.E_STATE and w.value == -7
    assert c.analyze(x, lens, "reference", cap=5)["ranges"] == base["ranges"]                        # still usable, and 5 is enough
    # a handle with another window: W = 30 ms at -40 dBFS against the definition
    c2 = cd.Conditioner(rate, min_silence_len=30, silence_thresh=-40)
    k2 = cd.threshold_k(-40)
    a = c2.analyze(x, lens, "both")
    for b in range(B):
        rg = cr.detect_silence(mono[b], rate, 30, k2)
        s, e, sliced = cr.kept_span(rg, cr.len_ms(len(mono[b]), rate), "both")
        assert a["ranges"][b] == rg and (int(a["s_ms"][b]), int(a["e_ms"][b])) == (s, e)
    c2.close()


def test_a_row_of_several_rounds_of_flag_words():
    """9.3 s at 8 kHz: 9,201 starts = 144 flag words, more than the 64 the range walk loads per lane position and round, beside a short row."""
    rate = 8000
    c = conditioner(rate)
    rows = [cc._row(rate, 9300, 41, "random", extra=cc.overhang(rate)), cc._row(rate, 350, 42, "lead")]
    assert (cr.len_ms(len(rows[0]), rate) - cc.W + 1 + 63) // 64 > 2 * 64
    x, lens = cr.batch(rows)
    for trim in ("reference", "both"):
        r = c.normalize(x, lens, trim=trim, loudness_dBFS=cc.TARGET_DBFS)
        for b, row in enumerate(rows):
            e = cr.normalize(row, rate, trim, cc.TARGET_DBFS)
            assert r["ranges"][b] == e["ranges"] and int(r["n_out"][b]) == e["n_out"] and r["gain"][b] == e["gain"]
            assert np.array_equal(r["pcm"][b, :e["n_out"]], e["pcm"]) and not r["pcm"][b, e["n_out"]:].any()
    assert len(r["ranges"][0]) > 20
