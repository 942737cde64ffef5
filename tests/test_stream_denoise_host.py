"""Host tests (no GPU) of the denoised vocoder stream (include/e2etts.h: e2etts_vocoder_stream_begin_denoised):
  * denoiser.stream_delay_frames against a brute-force dependency probe of the denoiser in float64 (tests/denoiser_ref.denoise_frames);
  * the window scheme restated in numpy (tests/stream_denoise_ref.py) against the whole-signal denoiser and the reference's fixture;
  * the new entry is named by the header, by _lib.EXPORTED_SYMBOLS and by the linker's version script.
Bit equality of the engine's stream with its one-shot denoiser is a GPU matter (tests/test_gpu_stream_denoise.py): float32 BLAS on the CPU
may block a short window's products differently from the whole signal's, hence 1e-6 here.
"""
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import denoiser_ref as dr
import stream_denoise_ref as sr
from e2e_tts_amd import _lib, denoiser as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ((1024, 4), (512, 2), (1024, 8), (256, 4))
CHUNKINGS = ([96], [1] * 96, [1, 7, 40, 3, 45], [50, 46])
_BASES = {}


def bases(N, V):
    if (N, V) not in _BASES:
        _BASES[(N, V)] = dn.stft_bases(N, N // V, N)
    return _BASES[(N, V)]


def test_delay_formula_values():
    assert dn.stream_delay_frames(1024, 256, 256) == 3     # the reference's defaults at the default hop_length
    assert dn.stream_delay_frames(1024, 256, 512) == 2     # ... at the 48 kHz config's
    assert dn.stream_delay_frames(256, 64, 256) == 1
    assert dn.stream_delay_frames(1024, 128, 256) == 4
    with pytest.raises(ValueError):
        dn.stream_delay_frames(1024, 256, 384)             # the denoiser hop must divide hop_length
    with pytest.raises(ValueError):
        dn.stream_delay_frames(1024, 341, 256)


@pytest.mark.parametrize("N,V", GEOMETRIES)
def test_delay_formula_against_a_dependency_probe(N, V):
    """Which output samples change when the tail x[E:], or the head x[:E], of a signal is replaced: a window whose right (left) edge is
    context at sample E knows nothing of x[E:] (x[:E]), so what it emits must lie before (after) every sample that changes."""
    hop = N // V
    fwd, inv, win_sq = bases(N, V)
    rng = np.random.Generator(np.random.PCG64(N + V))
    n = 8 * N
    x = rng.standard_normal(n) * 0.3
    bias = np.abs(rng.standard_normal(N // 2 + 1)) * 2.0
    base = dr.denoise_frames(x, bias, 0.1, fwd, inv, win_sq, hop)
    E = 4 * N
    xt, xh = x.copy(), x.copy()
    xt[E:] = rng.standard_normal(n - E)
    xh[:E] = rng.standard_normal(E)
    first = int(np.flatnonzero(dr.denoise_frames(xt, bias, 0.1, fwd, inv, win_sq, hop) != base)[0])
    lastc = int(np.flatnonzero(dr.denoise_frames(xh, bias, 0.1, fwd, inv, win_sq, hop) != base)[-1])
    print(f"({N}, {V}): replacing x[{E}:] first changes sample E - {E - first}; replacing x[:{E}] last changes sample E + {lastc - E}"
          f" (filter_length - hop = {N - hop})")
    assert E - first <= N - hop and lastc - E < N - hop   # the dependency the formula is built on
    for hl in (256, 512):
        if hl % hop:
            continue
        C = dn.stream_delay_frames(N, hop, hl)
        # right edge: samples before E - C * hl are emitted -- none of them may change, and no more than one frame is held back needlessly
        assert E - C * hl <= first < E - C * hl + hl + 1
        # left edge: samples from E + C * hl on are emitted
        assert E + C * hl > lastc >= E + C * hl - hl - 1


@pytest.mark.parametrize("N,V", GEOMETRIES)
def test_window_scheme_equals_the_whole_signal(N, V):
    hop, hl, T, halo = N // V, 256, 96, 2
    fwd, inv, win_sq = bases(N, V)
    C = dn.stream_delay_frames(N, hop, hl)
    rng = np.random.Generator(np.random.PCG64(7 * N + V))
    x = (rng.standard_normal(T * hl) * 0.2 + 0.05).astype(np.float32)
    bias = (np.abs(rng.standard_normal(N // 2 + 1)) * 2.0).astype(np.float32)
    for strength in (0.1, 0.0):
        whole = dr.denoise_rows(x, bias, strength, fwd, inv, win_sq, hop)
        for chunks in CHUNKINGS:
            pieces, lag = sr.denoise_stream(x, chunks, halo, C, hl, bias, strength, fwd, inv, win_sq, hop)
            got = np.concatenate(pieces)
            assert got.shape == whole.shape
            d = float(np.abs(got.astype(np.float64) - whole).max())
            assert d <= 1e-6, (chunks[:5], strength, d)
            # emitted frames lag pushed ones by halo + C until the last push, which emits everything
            for pushed, emitted in lag[:-1]:
                assert emitted == max(0, pushed - (halo + C))
            assert lag[-1] == (T, T)


def test_short_streams_pass_through_and_the_first_denoised_length():
    N, V, hl = 1024, 4, 256
    fwd, inv, win_sq = bases(N, V)
    rng = np.random.Generator(np.random.PCG64(3))
    bias = (np.abs(rng.standard_normal(N // 2 + 1))).astype(np.float32)
    for T in (1, 2):
        x = rng.standard_normal(T * hl).astype(np.float32)
        for chunks in ([T], [1] * T):
            pieces, _ = sr.denoise_stream(x, chunks, 2, 3, hl, bias, 0.1, fwd, inv, win_sq, N // V)
            np.testing.assert_array_equal(np.concatenate(pieces), x)
    x = rng.standard_normal(3 * hl).astype(np.float32)
    whole = dr.denoise_rows(x, bias, 0.1, fwd, inv, win_sq, N // V)
    for chunks in ([3], [1, 1, 1], [2, 1]):
        pieces, _ = sr.denoise_stream(x, chunks, 2, 3, hl, bias, 0.1, fwd, inv, win_sq, N // V)
        assert np.abs(np.concatenate(pieces) - whole).max() <= 1e-6


@pytest.mark.parametrize("tag", ("a", "b"))
@pytest.mark.parametrize("si", (0, 1))
def test_window_scheme_against_the_references_fixture(tag, si):
    """The fixture's audio cut into windows, against the reference's float64 output at the bars tests/test_gpu_denoiser.py holds the engine
    to: mean-L1 <= 4 x dref, max-abs <= 8 x dmax (the reference's own fp32-vs-float64 distances)."""
    gold = load_golden("denoiser")
    N, V = (int(v) for v in gold[f"{tag}_geometry"])
    hop = N // V
    fwd, inv, win_sq = bases(N, V)
    bias, s = gold[f"{tag}_bias"], float(gold[f"{tag}_strengths"][si])
    o64 = gold[f"{tag}_out64_s{si}"]
    dref, dmax = float(gold[f"{tag}_dref"][si]), float(gold[f"{tag}_dmax"][si])
    hl = hop          # the finest frame grid the stream allows: every valid length of the fixture is a multiple of it
    C = dn.stream_delay_frames(N, hop, hl)
    dist = []
    for b, nb in enumerate(int(v) for v in gold[f"{tag}_n_valid"]):
        if nb == 0:
            continue
        T = nb // hl
        chunks = [5] * (T // 5) + ([T % 5] if T % 5 else [])
        pieces, _ = sr.denoise_stream(gold[f"{tag}_audio"][b, :nb], chunks, 2, C, hl, bias, s, fwd, inv, win_sq, hop)
        got = np.concatenate(pieces)
        assert len(got) == nb
        if nb <= N // 2:
            np.testing.assert_array_equal(got, gold[f"{tag}_audio"][b, :nb])   # too short to reflect: copied through (the reference raises)
            continue
        dist.append(np.abs(got.astype(np.float64) - o64[b, :nb]))
    d = np.concatenate(dist)
    print(f"fixture {tag} ({N}, {V}) strength {s}: windows vs reference float64 mean-L1 {d.mean():.3e} (bar {4 * dref:.3e}) max {d.max():.3e} (bar {8 * dmax:.3e})")
    assert d.mean() <= 4 * dref and d.max() <= 8 * dmax


def test_the_new_entry_is_declared_exported_and_bound():
    name = "e2etts_vocoder_stream_begin_denoised"
    header = open(os.path.join(ROOT, "include", "e2etts.h")).read()
    assert re.search(r"^E2ETTS_API int " + name + r"\(e2etts_engine\* engine, int B, float strength, int\* delay_frames_out\);", header, re.M)
    assert "streaming denoise is out of scope" not in header
    assert name in _lib.EXPORTED_SYMBOLS and len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS)) == 39
    vmap = open(os.path.join(ROOT, "e2e_tts_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"^\s*([A-Za-z0-9_*?]+);", vmap.split("local:")[0], re.M)
    assert any(fnmatch.fnmatchcase(name, g) for g in globs), globs
