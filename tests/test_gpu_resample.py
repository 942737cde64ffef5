"""libe2etts_resample.so on the GPU: every output sample of the one-shot conversion against the float64 definition within the derived bar
(tests/resample_ref.py), the PCM rule, and the invariances the fixed-order sum gives bit for bit -- batch, chunking of a stream, call
order."""
import numpy as np
import pytest

import resample_ref as rr
from e2e_tts_amd import resample as rs

pytestmark = pytest.mark.gpu

RATIOS = [(2, 1), (1, 2), (3, 7), (160, 441), (320, 147), (147, 320), (1, 6)]   # (L, M)
_RS, _REF = {}, {}


def resampler(L, M):
    """One handle per ratio, shared by the tests: (3, 7) with a 2-zero filter, the others with the default design."""
    if (L, M) not in _RS:
        _RS[(L, M)] = rs.Resampler(M, L, zeros=2 if (L, M) == (3, 7) else 16)
    return _RS[(L, M)]


def read_device(res):
    """Host copy of a resident float32 tensor (a raw device address): the 1 / 1 conversion with the single tap 1.0 is an exact copy, and
    e2ers_forward reads device memory."""
    if "copy" not in _RS:
        _RS["copy"] = rs.Resampler(1, 1, taps=np.ones(1, np.float32))
    return _RS["copy"].forward(res, want=("wav",))["wav"]


def reference(L, M, x, nv):
    """(float64 outputs, bar) of one row, computed once per (ratio, signal, valid length)."""
    key = (L, M, x.dtype.name, x.size, int(nv), float(x[:8].astype(np.float64).sum()))
    if key not in _REF:
        taps = resampler(L, M).taps
        _REF[key] = (rr.resample_f64(x, taps, L, M, nv), rr.bar(x, taps, L, M, nv))
    return _REF[key]


def lengths(L, M):
    r = resampler(L, M)
    P = rr.taps_per_output(r.taps.size, L)
    edge = r.tile_outputs * M // L   # the input length whose outputs fill exactly one tile
    out = [1, max(2, P // 2), 3 * M, edge - 1, edge, edge + 1]
    if M > 1:
        out.append(3 * M + 1)        # n L not a multiple of M
    return sorted(set(out))


def check_rows(L, M, x, nvs, wav, lens, width, label):
    """Every sample of every row: inside the bar up to the row's n_out, zero from there to the layout width."""
    assert lens.tolist() == [rr.n_out(v, L, M) for v in nvs]
    for b, nv in enumerate(nvs):
        y, bar = reference(L, M, x[b], nv)
        got = wav[b, :len(y)].astype(np.float64)
        err = np.abs(got - y)
        worst = float((err / np.maximum(bar, 1e-300)).max()) if len(y) else 0.0
        print(f"{label} row {b} (n_valid {nv}, {len(y)} outputs): worst |gpu - float64| / bar = {worst:.3f}")
        assert np.isfinite(got).all() and (err <= bar).all(), (label, b, int(np.argmax(err - bar)))
        assert not wav[b, len(y):width].any(), (label, b, "samples past n_out are not 0")


@pytest.mark.parametrize("L,M", RATIOS)
def test_one_shot_every_sample_within_the_bar(L, M):
    import torch
    r = resampler(L, M)
    for n in lengths(L, M):
        W = rr.n_out(n, L, M)
        nvs = [n, n // 2, 0]
        # fp32, host arrays, dense
        x = np.stack([rr.make_signal(n, seed=10 * b + 1) for b in range(3)])
        out = r.forward(x, n_valid=nvs, want=("wav", "pcm"))
        assert out["width"] == W and out["wav"].shape == (3, W)
        check_rows(L, M, x, nvs, out["wav"], out["n_out"], W, f"{L}/{M} n={n} fp32 host")
        assert np.array_equal(out["pcm"], rr.pcm_of(out["wav"]))
        # int16, device tensors, strided input and output; the workspaces poisoned first
        r.poison_workspace()
        xi = np.stack([rr.make_signal(n, seed=10 * b + 2, dtype=np.int16) for b in range(3)])
        wide = torch.full((3, n + 9), 12345, dtype=torch.int16, device="cuda")
        wide[:, 3:3 + n] = torch.from_numpy(xi).cuda()
        stride = W + 5
        wav_d = torch.full((3, stride), 7.0, dtype=torch.float32, device="cuda")
        pcm_d = torch.full((3, stride), 7, dtype=torch.int16, device="cuda")
        out = r.forward(wide[:, 3:3 + n], n_valid=torch.tensor(nvs), out_wav=wav_d, out_pcm=pcm_d, out_stride=stride)
        wav_h, pcm_h = wav_d.cpu().numpy(), pcm_d.cpu().numpy()
        check_rows(L, M, xi, nvs, wav_h, out["n_out"], W, f"{L}/{M} n={n} int16 device strided")
        assert (wav_h[:, W:] == 7.0).all() and (pcm_h[:, W:] == 7).all()      # the columns between the rows are not touched
        assert np.array_equal(pcm_h[:, :W], rr.pcm_of(wav_h[:, :W]))
        # the resident outputs are this call's, dense
        rw, rp = r.resident()
        assert rw.shape == (3, W) and rp.shape == (3, W)
        back = read_device(rw)
        assert np.array_equal(back, wav_h[:, :W])


def test_pcm_saturates_on_a_full_scale_square_wave():
    """48000 -> 8000: a full-scale int16 square wave overshoots 1.0 after the low-pass (Gibbs), so both rails are exercised."""
    L, M = 1, 6
    r = resampler(L, M)
    n = 6000
    period = 96     # 500 Hz at 48 kHz: several harmonics inside the 4 kHz band
    x = np.where((np.arange(n) // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)
    y64, _ = reference(L, M, x, n)
    assert y64.max() > 1.0 and y64.min() < -1.0, "the reference itself must leave [-1, 1] for saturation to be exercised"
    out = r.forward(x[None, :], want=("wav", "pcm"))
    wav, pcm = out["wav"][0], out["pcm"][0]
    assert wav.max() > 1.0 and wav.min() < -1.0
    assert np.array_equal(pcm, rr.pcm_of(wav))
    assert pcm.max() == 32767 and pcm.min() == -32768
    assert (pcm[wav >= 1.0] == 32767).all() and (pcm[wav <= -1.0] == -32768).all()


@pytest.mark.parametrize("L,M", [(320, 441), (147, 320), (1, 6)])
def test_batch_row_equals_single_row_bit_for_bit(L, M):
    r = resampler(L, M)
    n = r.tile_outputs * M // L + 37
    x = np.stack([rr.make_signal(n, seed=30 + b) for b in range(3)])
    nvs = [n, n - 501, 13]
    full = r.forward(x, n_valid=nvs, want=("wav", "pcm"))
    for b in range(3):
        one = r.forward(x[b:b + 1], n_valid=nvs[b:b + 1], want=("wav", "pcm"))
        assert np.array_equal(one["wav"][0], full["wav"][b]) and np.array_equal(one["pcm"][0], full["pcm"][b])
        # and a row cut to its valid length is the same conversion
        cut = r.forward(x[b:b + 1, :nvs[b]], want=("wav",))
        assert np.array_equal(cut["wav"][0], full["wav"][b, :cut["width"]])


def chunkings(n, history):
    ones = [1] * n
    primes, k = [], 0
    while sum(primes) < n:
        primes.append(min((7, 13, 251)[k % 3], n - sum(primes)))
        k += 1
    long_then_flush = [n, 0]   # one chunk longer than the history, then `last` with n = 0
    assert n > history
    return {"ones": ones, "primes": primes, "long_then_flush": long_then_flush}


@pytest.mark.parametrize("L,M", [(320, 441), (147, 320), (2, 1), (1, 6)])
def test_stream_equals_one_shot_for_any_chunking(L, M):
    import torch
    r = resampler(L, M)
    P = rr.taps_per_output(r.taps.size, L)
    n = 2 * P + 700
    for dtype in (np.float32, np.int16):
        x = np.stack([rr.make_signal(n, seed=50 + b, dtype=dtype) for b in range(2)])
        want = r.forward(x, want=("wav", "pcm"))
        for name, sizes in chunkings(n, P).items():
            if name == "ones" and dtype == np.int16:
                continue   # (covered in fp32; one launch per sample)
            cuts = np.cumsum([0] + sizes)
            pieces = [x[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
            # two pushes in flight (the generator pushes chunk i + 1 before it fetches chunk i); device chunks for the primes
            feed = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pieces] if name == "primes" else pieces
            got = list(r.stream(feed, want_pcm=dtype == np.int16))
            cat = np.concatenate(got, axis=1)
            assert np.array_equal(cat, want["pcm"] if dtype == np.int16 else want["wav"]), (L, M, name, "generator")
            # push, then fetch at once
            r.stream_begin(2, rs.F32 if dtype == np.float32 else rs.I16)
            got = []
            for i, p in enumerate(pieces):
                made = r.stream_push(p if p.shape[1] else None, last=i == len(pieces) - 1)
                if made:
                    got.append(r.stream_fetch(2, made))
            assert np.array_equal(np.concatenate(got, axis=1), want["wav"]), (L, M, name, "push then fetch")
        # a third unfetched push is refused, and the stream goes on after a fetch
        r.stream_begin(2, rs.F32 if dtype == np.float32 else rs.I16)
        a = r.stream_push(x[:, :P + 300])
        b = r.stream_push(x[:, P + 300:P + 500])
        assert a > 0 and b > 0
        with pytest.raises(RuntimeError):
            r.stream_push(x[:, P + 500:], last=True)
        first = r.stream_fetch(2, a)
        c = r.stream_push(x[:, P + 500:], last=True)
        rest = [r.stream_fetch(2, b), r.stream_fetch(2, c)]
        assert np.array_equal(np.concatenate([first] + rest, axis=1), want["wav"])
        with pytest.raises(RuntimeError):
            r.stream_push(x[:, :5])          # after the last chunk
        with pytest.raises(RuntimeError):
            r.stream_fetch(2, 1)             # nothing unfetched


def test_stream_of_vocoder_pieces_equals_one_shot():
    """48000 -> 22050 over the long-form stream's pieces: 512 frames of hop 512 each, the last one short; a one-shot call between two
    steps does not disturb the stream."""
    L, M = 147, 320
    r = resampler(L, M)
    piece = 512 * 512
    n = 2 * piece + 12345
    x = rr.make_signal(n, seed=77)[None, :]
    want = r.forward(x, want=("wav",))["wav"]
    pieces = [x[:, a:min(n, a + piece)] for a in range(0, n, piece)]
    got = []
    for i, out in enumerate(r.stream(pieces)):
        got.append(out)
        if i == 0:
            r.forward(x[:, :1000], want=())
    assert np.array_equal(np.concatenate(got, axis=1), want)
    # spot check of the whole against the definition: the outputs around the two piece borders and the end
    E = [rr.emitted(k * piece, L, M, (r.taps.size - 1) // 2) for k in (1, 2)]
    ms = np.unique(np.concatenate([np.arange(max(0, e - 40), e + 40) for e in E] + [np.arange(want.shape[1] - 80, want.shape[1])]))
    y = rr.resample_f64(x[0], r.taps, L, M, ms=ms)
    assert (np.abs(want[0, ms] - y) <= rr.bar(x[0], r.taps, L, M, ms=ms)).all()


def test_positions_past_int32():
    """22050 -> 16000 on 7,000,000 samples: c(m) = m M + half passes 2^31 before the end of the row (the smallest case that overflows int32);
    the last 4096 outputs against the definition."""
    L, M = 320, 441
    r = resampler(L, M)
    n = 7_000_000
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.integers(-30000, 30000, size=n, dtype=np.int16)
    W = rr.n_out(n, L, M)
    half = (r.taps.size - 1) // 2
    assert (W - 4096) * M + half > 2 ** 31
    out = r.forward(x[None, :], want=("wav",))
    assert out["width"] == W and out["n_out"].tolist() == [W]
    ms = np.arange(W - 4096, W)
    y = rr.resample_f64(x, r.taps, L, M, ms=ms)
    bar = rr.bar(x, r.taps, L, M, ms=ms)
    err = np.abs(out["wav"][0, ms].astype(np.float64) - y)
    print(f"last 4096 of {W} outputs: worst |gpu - float64| / bar = {float((err / bar).max()):.3f}")
    assert (err <= bar).all()
    head = np.arange(0, 2048)   # and the start of the row, where everything still fits int32
    assert (np.abs(out["wav"][0, head] - rr.resample_f64(x, r.taps, L, M, ms=head)) <= rr.bar(x, r.taps, L, M, ms=head)).all()


def test_failed_load_keeps_the_filter_and_einval_keeps_the_outputs():
    import torch
    L, M = 3, 7
    r = rs.Resampler(M, L, zeros=2)
    n = 500
    x = rr.make_signal(n, seed=3)[None, :]
    first = r.forward(x, want=("wav", "pcm"))
    lib, h = r.lib, r._h
    bad = r.taps.copy()
    bad[3] = np.inf
    assert lib.e2ers_load(h, bad.ctypes.data, bad.size, L, M) == rs.E_INVAL                  # a tap that is not finite
    assert lib.e2ers_load(h, r.taps.ctypes.data, r.taps.size - 1, L, M) == rs.E_INVAL        # an even count
    assert lib.e2ers_load(h, r.taps.ctypes.data, r.taps.size, 6, 14) == rs.E_INVAL           # not in lowest terms
    r.resident()                                                                              # still resident: nothing was enqueued
    again = r.forward(x, want=("wav", "pcm"))
    assert np.array_equal(again["wav"], first["wav"]) and np.array_equal(again["pcm"], first["pcm"])

    def resident_copy():
        return read_device(r.resident()[0])

    before = resident_copy()
    assert np.array_equal(before, first["wav"])
    W = first["width"]
    small = np.zeros((1, W), np.float32)
    with pytest.raises(ValueError):
        r.forward(x, n_valid=[n + 1])                                                         # n_valid > n
    with pytest.raises(ValueError):
        r._check(lib.e2ers_forward(h, x.ctypes.data, rs.F32, n, None, 1, n, small.ctypes.data, None, W - 1, None, None), "e2ers_forward")   # out_stride < width
    with pytest.raises(ValueError):
        r._check(lib.e2ers_forward(h, x.ctypes.data, 5, n, None, 1, n, small.ctypes.data, None, W, None, None), "e2ers_forward")
    assert not small.any()
    assert np.array_equal(resident_copy(), before)
    # a new filter for the same handle replaces the old one and forgets the outputs
    taps2 = rs.design(M, L, zeros=3)[0]
    assert lib.e2ers_load(h, taps2.ctypes.data, taps2.size, L, M) == rs.E_OK
    with pytest.raises(RuntimeError):
        r.resident()
    r.taps = taps2
    out = r.forward(x, want=("wav",))
    y = rr.resample_f64(x[0], taps2, L, M)
    assert (np.abs(out["wav"][0] - y) <= rr.bar(x[0], taps2, L, M)).all()
    assert r.device_bytes() > 0
    r.profile_enable(True)
    r.forward(x, want=())
    assert set(r.profile_read()) == {"upload", "filter", "fetch"}
    r.close()
