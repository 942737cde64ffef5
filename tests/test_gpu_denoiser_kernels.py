"""Per-kernel tests (-m gpu) of the seven passes of csrc/denoiser.hip -- reflect-pad, spectral subtraction, bias frame, overlap-add
normalisation, their stream forms and the table fill -- one launch wrapper at a time through tests/csrc/denoiser_harness.hip
(tests/denoiser_harness.py), at the shapes and values of tests/denoiser_kernel_cases.py.

One tier, exact: every operation of these kernels is a selection, one correctly rounded IEEE operation or an integer decision, so every
output element must be BIT-EQUAL to the numpy float32 restatement of tests/denoiser_kernel_ref.py (two NaNs count as equal).  Buffers follow
tests/test_gpu_kernels.py: every device buffer is a view between guard bands (Guarded), strided inputs have NaN in their row gaps, outputs
are pre-filled with a sentinel, bands and gaps must hold their bits afterwards, and "left alone" means the sentinel survives.

Every test counts (launches, elements compared, elements differing) into a tally that the last test prints and records, so a run on other
kernels reports by how much each family departs."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoiser_kernel_cases as dc   # noqa: E402
import denoiser_kernel_ref as dr     # noqa: E402
from test_gpu_kernels import Guarded, i32, record   # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT = f32(-12345.5)
PSENT = np.int16(-31111)
_T0 = time.time()
_tally = {}


@pytest.fixture(scope="module")
def dh():
    import torch
    assert torch.cuda.is_available(), "the kernel tests need the GPU"
    import denoiser_harness
    import __graft_entry__ as g
    assert g.built_harness_denoiser_hash() == g.harness_denoiser_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    denoiser_harness.load()
    assert g.harness_denoiser_hash() in denoiser_harness.version()
    return denoiser_harness


def judge(family, got, want):
    """Counts the differing elements into the tally, then asserts there are none."""
    nd = dr.diff_count(got, want)
    t = _tally.setdefault(family, [0, 0, 0])
    t[0] += 1
    t[1] += int(np.asarray(want).size)
    t[2] += nd
    assert nd == 0, f"{family}: {nd} of {np.asarray(want).size} elements differ from the restatement"


class Flat:
    """`count` elements at an offset of `off` elements into a guarded allocation: off = 0 is 16-byte aligned, off = 1 is not.  data: an input
    (must stay unchanged); otherwise an output filled with the sentinel, judged through fetch()."""

    def __init__(self, data=None, count=None, off=0, dtype=np.float32, sentinel=SENT):
        if data is not None:
            data = np.ascontiguousarray(data).reshape(-1)
            count, dtype = data.size, data.dtype
        host = np.full(off + count, sentinel, dtype)
        if data is not None:
            host[off:] = data
            if off:
                host[:off] = np.nan if np.dtype(dtype).kind == "f" else -1
        self.g, self.off, self.count = Guarded(host) if data is not None else Guarded(shape=(off + count,), dtype=dtype, sentinel=dtype(sentinel)), off, count
        self.ptr = self.g.ptr + off * np.dtype(dtype).itemsize
        self.sentinel = sentinel

    def fetch(self, shape):
        body, ok = self.g.fetch()
        body = body.reshape(-1)
        assert ok, "a guard band was written"
        assert np.all(body[:self.off] == self.sentinel), "the elements before an unaligned output were written"
        return body[self.off:].reshape(shape)

    def unchanged(self):
        return self.g.unchanged()


def rows(data, stride, off=0):
    """[B, C] rows at row stride `stride` >= C (NaN in the gaps), the first at an offset of `off` elements: flat, for the Flat input."""
    data = np.asarray(data)
    B, C = data.shape
    flat = np.full(B * stride, np.nan, data.dtype)
    flat.reshape(B, stride)[:, :C] = data
    return Flat(flat, off=off)


def unchanged(*gs):
    for g in gs:
        assert g is None or g.unchanged(), "an input buffer or its guard band was written"


# ---------------------------------------------------------------- reflect-pad
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_stft_pad(dh, N, hop):
    """n_valid = half (zeros), half + 1, a length off the float4 grid; R larger than needed; the aligned vector path and the scalar path (odd
    row stride, base pointer off 16 bytes) on the same data."""
    c = dc.pad_case(N, hop)
    B, R, wl = 3, c["R"], c["wav"].shape[1]
    want = dr.stft_pad_ref(c["wav"], c["n_valid"], R, N, hop)
    nv = i32(c["n_valid"])
    for stride, off in (((wl + 3) // 4 * 4, 0), ((wl + 3) // 4 * 4 + 1, 1)):
        gw, go = rows(c["wav"], stride, off), Flat(count=B * R * hop)
        assert dh.stft_pad(gw.ptr, stride, nv.data_ptr(), go.ptr, B, R, N, hop) is None
        judge("stft_pad", go.fetch((B, R * hop)), want)
        unchanged(gw)
    assert not want[0].any() and want[1].any()


@pytest.mark.parametrize("left,right", dc.EDGES)
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_stft_pad_stream(dh, N, hop, left, right):
    """All four edge combinations at the shortest window with a real edge (half + hop) and a longer one; aligned and unaligned seg."""
    for L in (N // 2 + hop, 2 * N + hop):
        c = dc.stream_pad_case(N, hop, left, right, L)
        want = dr.stft_pad_stream_ref(c["seg"], L, N, hop, left, right)
        assert want.shape == (2, c["Rq"] * hop)
        for stride, off in ((L, 0), (L + 3, 1)):
            gs, go = rows(c["seg"], stride, off), Flat(count=2 * c["Rq"] * hop)
            assert dh.stft_pad_stream(gs.ptr, stride, go.ptr, 2, L, c["Rq"], N, hop, left, right) is None
            judge("stft_pad_stream", go.fetch(want.shape), want)
            unchanged(gs)


def test_stft_pad_stream_refuses_a_window_off_the_hop_grid(dh):
    """L = half + 1 cannot be launched: the rows must match the window, so L is a multiple of hop."""
    msg = dh.stft_pad_stream(0x10000, 40, 0x10000, 1, 33, 3, 64, 32, True, True)
    assert isinstance(msg, str) and "rows do not match" in msg, msg


# ---------------------------------------------------------------- spectral subtraction, bias frame
@pytest.mark.parametrize("strength", dc.STRENGTHS)
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_spectral_subtract(dh, N, hop, strength):
    c = dc.spec_case(N, hop, strength)
    B, R, Cpad, bins, nov = 3, c["R"], c["Cpad"], c["bins"], c["nov"]
    held = c["spec"].copy()
    for b, Fb in enumerate(c["frames"]):
        held[b, Fb + nov - 1:] = SENT                                  # rows the launch must leave alone
    want = dr.spectral_subtract_ref(held, c["bias"], c["frames"], N, nov, strength)
    gs, gb, fr = Flat(held), Flat(c["bias"]), i32(c["frames"])
    assert dh.spectral_subtract(gs.ptr, gb.ptr, fr.data_ptr(), B, R, Cpad, N, nov, strength) is None
    got = gs.g.fetch()[0].reshape(B, R, Cpad)
    assert gs.g.fetch()[1], "a guard band was written"
    unchanged(gb)
    for b, Fb in enumerate(c["frames"]):                               # the restatement's own structure, stated once more
        assert not want[b, Fb:Fb + nov - 1].any() and np.all(want[b, Fb + nov - 1:] == SENT) and not want[b, :Fb, 2 * bins:].any()
    if strength == 0:                                                  # md == mag, sc == 1: the input's bits wherever mag > 0
        for b, Fb in enumerate(c["frames"]):
            re, im = held[b, :Fb, :bins], held[b, :Fb, bins:2 * bins]
            pos = dr.magnitude_ref(re, im) > 0
            pos &= np.isfinite(dr.magnitude_ref(re, im))
            assert np.array_equal(dr.bits(got[b, :Fb, :bins])[pos], dr.bits(re)[pos]) and np.array_equal(dr.bits(got[b, :Fb, bins:2 * bins])[pos], dr.bits(im)[pos])
    judge(f"spectral_subtract s={strength:g}", got, want)


@pytest.mark.parametrize("N", [64, 1024, 131070])
def test_bias_frame(dh, N):
    """bins 33 and 513 (and 65536: the root over 40 decades); the element after `bins` is a guard band."""
    bins = N // 2 + 1
    row = dc.bias_case(N)
    gr, gb = Flat(row), Flat(count=bins)
    assert dh.bias_frame(gr.ptr, gb.ptr, N) is None
    judge("bias_frame", gb.fetch((bins,)), dr.magnitude_ref(row[:bins], row[bins:]))
    unchanged(gr)


# ---------------------------------------------------------------- overlap-add normalisation
def _ola(dh, N, hop, c, odd, want_wav, want_pcm, want):
    B, n, R = 3, c["n"], c["R"]
    gy, gi, gw_sq = Flat(c["y"]), rows(c["inp"], n + 3, 1 if odd else 0), Flat(c["win_sq"])
    nv, fr = i32(c["n_valid"]), i32(c["frames"])
    off = 1 if odd else 0
    gw = Flat(count=B * n, off=off) if want_wav else None
    gp = Flat(count=B * n, off=off, dtype=np.int16, sentinel=PSENT) if want_pcm else None
    assert dh.ola_norm(gy.ptr, gi.ptr, n + 3, nv.data_ptr(), fr.data_ptr(), gw_sq.ptr, gw.ptr if gw else None, gp.ptr if gp else None, B, n, R, N, hop) is None
    wav = None
    if want_wav:
        wav = gw.fetch((B, n))
        judge("ola_norm wav", wav, want)
    if want_pcm:
        judge("ola_norm pcm", gp.fetch((B, n)), dr.pcm_ref(want))
    unchanged(gy, gi, gw_sq)
    return wav


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("N,hop", dc.GEOMS)
def test_ola_norm(dh, N, hop, holes):
    """Full, ragged and pass-through rows; the vector path (n % 4 == 0, aligned) and the scalar path (n % 4 == 1, wav and pcm off their
    alignment); wav only, pcm only, both; holes: a window whose envelope is 0 or under FLT_MIN on stretches (not divided); the PCM rails."""
    for odd in (False, True):
        c = dc.ola_case(N, hop, holes, odd)
        want = dr.ola_norm_ref(c["y"], c["inp"], c["n_valid"], c["frames"], c["win_sq"], c["n"], N, hop)
        assert not want[1, c["n_valid"][1]:].any() and np.array_equal(dr.pcm_ref(want[2, 2:9]), dc.PCM_RAILS_WANT)
        if holes:
            assert np.array_equal(dr.pcm_ref(want[0, 2 * hop:2 * hop + 7]), dc.PCM_RAILS_WANT)
        for want_wav, want_pcm in ((True, True), (True, False), (False, True)):
            _ola(dh, N, hop, c, odd, want_wav, want_pcm, want)


@pytest.mark.parametrize("N,hop", dc.SMALL_GEOMS)
def test_ola_norm_stream_pieces_equal_the_whole(dh, N, hop):
    """The same overlap-add emitted in three pieces (a vector one, an odd scalar one, the rest; the end unknown for the early ones) equals
    launch_ola_norm's samples and the restatement bit for bit."""
    half, nov, B = N // 2, N // hop, 2
    n = 8 * hop
    F, R = n // hop + 1, n // hop + nov
    r = dc.rng_of(f"dn_stream_{N}")
    y = r.standard_normal((B, R * hop)).astype(f32)
    win = dc.window_sq(N, hop, False)
    gy, gi, gq = Flat(y), Flat(np.full((B, n), np.nan, f32)), Flat(win)
    nv, fr = i32([n] * B), i32([F] * B)
    gw = Flat(count=B * n)
    assert dh.ola_norm(gy.ptr, gi.ptr, n, nv.data_ptr(), fr.data_ptr(), gq.ptr, gw.ptr, None, B, n, R, N, hop) is None
    whole = gw.fetch((B, n))
    judge("ola_norm wav", whole, dr.ola_norm_ref(y, np.zeros((B, n), f32), [n] * B, [F] * B, win, n, N, hop))
    i0 = 0
    for k, m in enumerate((3 * hop, 5, n - 3 * hop - 5)):
        last = k == 2
        assert last or (i0 + m - 1 + half) // hop <= F - 1            # an unknown end is allowed only where the clamp cannot bind
        F_abs = F if last else dr.LLONG_MAX
        gw, gp = Flat(count=B * m), Flat(count=B * m, dtype=np.int16, sentinel=PSENT)
        assert dh.ola_norm_stream(gy.ptr, R * hop, i0 + half, gi.ptr, n, gq.ptr, gw.ptr, gp.ptr, B, m, i0 + half, F_abs, N, hop, False) is None
        piece = gw.fetch((B, m))
        judge("ola_norm_stream wav", piece, whole[:, i0:i0 + m])
        judge("ola_norm_stream wav", piece, dr.ola_norm_stream_ref(y, i0 + half, None, win, m, i0 + half, F_abs, N, hop, False))
        judge("ola_norm_stream pcm", gp.fetch((B, m)), dr.pcm_ref(whole[:, i0:i0 + m]))
        i0 += m
    unchanged(gy, gi, gq)


@pytest.mark.parametrize("known_end", [False, True])
@pytest.mark.parametrize("N,hop", dc.SMALL_GEOMS + [(1024, 256)])
def test_ola_norm_stream_past_2_to_33(dh, N, hop, known_end):
    """p_abs0 a multiple of hop just above 2^33: the frame range and the window index in 64-bit arithmetic, against Python integers; a known
    end two frames into the piece (the clamp binds) against F_abs = LLONG_MAX."""
    B, n, y_off = 2, 3 * hop + 2, 5
    p_abs0 = (2 ** 33 // hop + 3) * hop
    F_abs = p_abs0 // hop + 2 if known_end else dr.LLONG_MAX
    r = dc.rng_of(f"dn_stream33_{N}")
    y = r.standard_normal((B, n + y_off + 3)).astype(f32)
    for holes in (False, True):
        win = dc.window_sq(N, hop, holes)
        gy, gi, gq, gw = Flat(y), Flat(np.full((B, n), np.nan, f32)), Flat(win), Flat(count=B * n, off=1)
        assert dh.ola_norm_stream(gy.ptr, y.shape[1], y_off, gi.ptr, n, gq.ptr, gw.ptr, None, B, n, p_abs0, F_abs, N, hop, False) is None
        want = dr.ola_norm_stream_ref(y, y_off, None, win, n, p_abs0, F_abs, N, hop, False)
        judge("ola_norm_stream wav", gw.fetch((B, n)), want)
        unchanged(gy, gi, gq)
    if known_end:     # the clamp changed something: the tail of the piece has fewer frames than with the end unknown
        assert dr.diff_count(want, dr.ola_norm_stream_ref(y, y_off, None, win, n, p_abs0, dr.LLONG_MAX, N, hop, False)) > 0


def test_ola_norm_stream_pass(dh):
    """pass = true: in copied (the rails through the PCM conversion), y absent."""
    N, hop, B, n = 64, 32, 2, 29
    inp = dc.rng_of("dn_stream_pass").standard_normal((B, n)).astype(f32)
    inp[1, 3:10] = (dc.PCM_RAILS / 32768).astype(f32)
    gi, gq = rows(inp, n + 2, 1), Flat(dc.window_sq(N, hop, False))
    gw, gp = Flat(count=B * n), Flat(count=B * n, dtype=np.int16, sentinel=PSENT)
    assert dh.ola_norm_stream(None, 0, 0, gi.ptr, n + 2, gq.ptr, gw.ptr, gp.ptr, B, n, 12345 * hop, 1, N, hop, True) is None
    judge("ola_norm_stream wav", gw.fetch((B, n)), inp)
    judge("ola_norm_stream pcm", gp.fetch((B, n)), dr.pcm_ref(inp))
    unchanged(gi, gq)


@pytest.mark.parametrize("n", [1, 257])
def test_fill_i32(dh, n):
    g = Flat(count=n, dtype=np.int32, sentinel=np.int32(-777))
    assert dh.fill_i32(g.ptr, n, -123456789) is None
    judge("fill_i32", g.fetch((n,)), np.full(n, -123456789, np.int32))


def test_tally_and_wall_time():
    """Launches judged, elements compared and elements differing per family, and the module's wall time: printed and recorded."""
    for fam, (launches, elems, nd) in sorted(_tally.items()):
        print(f"[denoiser kernels] {fam}: {launches} comparisons, {elems} elements, {nd} differing")
        record("denoiser_kernels", kernel=fam, comparisons=launches, elements=elems, differing=nd)
    record("denoiser_kernels_wall", seconds=time.time() - _T0)
    print(f"[denoiser kernels] wall time {time.time() - _T0:.1f} s")
