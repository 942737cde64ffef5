"""Seeded generators of the conditioning case matrix: every row is rebuilt from its recipe, so tests/golden/condition_cases.npz holds only
what audioop gave for it.  A row is laid out per millisecond (samples [pos(p), pos(p + 1)) of ms p): "loud" ms are uniform noise of
+-8000, "quiet" ms noise of +-40, "zero" ms zeros, and a "blip" ms is the constant 870: one blip in a window is ~0.7 of the silence
threshold's energy, two are ~1.4 -- windows that hold one are silent, windows that hold two are not, which isolates single silent starts."""
import numpy as np

import condition_ref as cr

LOUD, QUIET, ZERO, BLIP = 0, 1, 2, 3
TARGET_DBFS = -20.0
W = cr.W_DEFAULT


def render(kinds, rate, extra, seed):
    """kinds [n_ms] -> int16 samples of pos(n_ms) + extra frames (the extra ones loud)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_ms = len(kinds)
    N = cr.pos(n_ms, rate) + extra
    per = np.full(N, LOUD, np.int8)
    for p in range(n_ms):
        per[cr.pos(p, rate):cr.pos(p + 1, rate)] = kinds[p]
    x = rng.integers(-8000, 8001, N)
    q = rng.integers(-40, 41, N)
    x = np.where(per == QUIET, q, x)
    x = np.where(per == ZERO, 0, x)
    x = np.where(per == BLIP, 870, x)
    return x.astype(np.int16)


def random_kinds(n_ms, seed):
    """Alternating quiet / loud stretches around the window length"""
    rng = np.random.Generator(np.random.PCG64(seed))
    kinds = np.empty(n_ms, np.int8)
    p, quiet = 0, bool(rng.integers(0, 2))
    while p < n_ms:
        d = int(rng.choice([30, 90, 100, 101, 150, 199, 200, 201, 250, 400]))
        kinds[p:p + d] = QUIET if quiet else LOUD
        p += d
        quiet = not quiet
    return kinds


def edge_kinds(n_ms, T):
    """Ranges and merges across the edges of the window test's tiles of T starts (n_ms >= 3 T + 400):
    a quiet stretch over the first edge; at the second edge a silent start exactly W after its predecessor (one range); at the third
    one W + 1 after (two ranges); a quiet tail, so the last range ends at len_ms."""
    assert n_ms >= 3 * T + 400 and T >= 3 * W
    kinds = np.full(n_ms, LOUD, np.int8)
    kinds[T - 60:T + 190] = QUIET                       # silent starts T - 60 .. T + 90
    a = 2 * T - 24                                      # silent a, then a + W, a + W + 1, ...: merged
    kinds[a:a + 2 * W + 40] = ZERO
    kinds[a + W - 1] = kinds[a + W] = BLIP
    a = 3 * T - 36                                      # silent a, then a + W + 1, ...: split
    kinds[a:a + 2 * W + 40] = ZERO
    kinds[a + W - 1] = kinds[a + W] = kinds[a + W + 1] = BLIP
    kinds[n_ms - 130:] = QUIET
    return kinds


def overhang(rate):
    """Extra frames after a whole number of ms that make len_ms round up: pos(len_ms) > N"""
    per = rate / 1000.0
    e = int(per * 0.5) + 1
    assert e < per
    return e


def _row(rate, n_ms, seed, kind="random", extra=0, T=512):
    if kind == "random":
        kinds = random_kinds(n_ms, seed)
    elif kind == "edge":
        kinds = edge_kinds(n_ms, T)
    elif kind == "quiet":
        kinds = np.full(n_ms, QUIET, np.int8)
    elif kind == "lead":   # silence, speech, silence: what a studio recording looks like
        kinds = np.full(n_ms, LOUD, np.int8)
        kinds[:n_ms // 3] = QUIET
        kinds[n_ms - n_ms // 4:] = QUIET
    else:
        raise ValueError(kind)
    return render(kinds, rate, extra, seed)


def _stereo(rate, n_ms, seed, kind, extra=0):
    """[N, 2]: two renderings of one layout with different noise (odd sums exercise the floor of the downmix)"""
    l, r = _row(rate, n_ms, seed, kind, extra), _row(rate, n_ms, seed + 1000, kind, extra)
    return np.stack([l, r], 1)


def cases(T=512):
    """name -> dict(rate, channels, rows): rows are [N] int16 (mono) or [N, 2] (stereo).  T: starts per tile of the window test (the
    edge rows are laid out around its multiples; the goldens are recorded for 512 = choose_tile(100))."""
    return {
        "r8000": dict(rate=8000, channels=1, rows=[
            _row(8000, 99, 11, "quiet"),                     # no analysis
            _row(8000, 100, 12, "quiet"),                    # exactly one window
            _row(8000, 101, 13, "lead"),
            _row(8000, 350, 14, "random", extra=overhang(8000)),
            _row(8000, 3 * T + 1060, 15, "edge")]),
        "r22050": dict(rate=22050, channels=1, rows=[
            _row(22050, 352, 21, "lead", extra=overhang(22050)),
            _row(22050, 3 * T + 1064, 22, "edge", extra=overhang(22050)),
            _row(22050, 99, 23, "random"),
            _row(22050, 1300, 24, "quiet")]),                # all silent
        "r44100s": dict(rate=44100, channels=2, rows=[
            _stereo(44100, 3 * T + 1070, 31, "random", extra=overhang(44100)),
            _stereo(44100, 350, 32, "lead"),
            _stereo(44100, 101, 33, "quiet")]),
    }


def mono_rows(case):
    return [cr.downmix(r) if case["channels"] == 2 else r for r in case["rows"]]
