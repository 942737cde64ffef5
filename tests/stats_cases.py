"""The seeded cases of the corpus-statistics tests (tests/test_stats_host.py, tests/test_gpu_stats.py) and of the fixture
tools/make_stats_goldens.py writes (tests/golden/stats_cases.npz): rows of frame values by length, ragged batches, constant rows,
tie-rich integer rows, rows with heavy outliers, rows in which a value equals a fence exactly, f0 tracks, and a corpus of twelve rows.

A corpus is a list of utterances, each a dict of three float32 rows: "energy", "pitch" (any scaled track) and "f0" (Hz, 0 = unvoiced).
The fixture holds what the reference's own text computed on them and a digest of every corpus, so a generator that drifted is noticed."""
import hashlib
import os
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_cases.npz")
CAP = 16384   # E2EST_MAX_ROW
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1025, CAP)
STAT_KEYS = ("f0.mean", "f0.std", "pitch.max", "pitch.min", "pitch.mean", "pitch.std", "energy.max", "energy.min", "energy.mean", "energy.std")


def rng_of(name: str) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def tri(t) -> np.ndarray:
    """A triangle wave of period 2 in [0, 1]: a contour made of correctly rounded operations only (the rows are the same on every CPU)."""
    return np.abs(np.mod(t, 2.0) - 1.0)


def energy_row(rng, n: int) -> np.ndarray:
    """Frame energies as the mel front-end gives them: positive, skewed, a slow contour under frame noise."""
    y = 1.0 + 0.5 * tri(np.arange(n) / 37.0 + rng.uniform(0, 2.0)) + 0.3 * rng.standard_normal(n)
    return (y * y * rng.uniform(5.0, 40.0)).astype(np.float32)


def pitch_row(rng, n: int) -> np.ndarray:
    """A scaled pitch track: continuous, positive, a few halving / doubling errors as outliers."""
    x = 180.0 + 40.0 * tri(np.arange(n) / 23.0 + rng.uniform(0, 2.0)) + 6.0 * rng.standard_normal(n)
    x[rng.random(n) < 0.03] *= 2.0
    x[rng.random(n) < 0.03] *= 0.5
    return x.astype(np.float32)


def f0_row(rng, n: int, kind: str = "mixed") -> np.ndarray:
    """An f0 track in Hz, 0 = unvoiced; "mixed" holds voiced and unvoiced stretches and, from 4 frames on, one -0.0 (unvoiced)."""
    x = (120.0 + 50.0 * tri(np.arange(n) / 29.0 + rng.uniform(0, 2.0)) + 3.0 * rng.standard_normal(n)).astype(np.float32)
    if kind == "unvoiced":
        x[:] = 0.0
    elif kind == "mixed":
        uv = tri(np.arange(n) / 5.0 + rng.uniform(0, 2.0)) > 0.6
        x[uv] = 0.0
        if n >= 4:
            x[n // 2] = -0.0
    return x


def utterance(name: str, n: int, f0_kind: str = "mixed") -> dict:
    rng = rng_of(name)
    return {"energy": energy_row(rng, n), "pitch": pitch_row(rng, n), "f0": f0_row(rng, n, f0_kind)}


def heavy_outliers(name: str, n: int) -> dict:
    u = utterance(name, n)
    rng = rng_of(name + "/out")
    for k in ("energy", "pitch"):
        idx = rng.choice(n, max(1, n // 10), replace=False)
        u[k][idx] *= rng.choice(np.array([1e-3, 1e3, -50.0], np.float32), idx.size)
    return u


def integer_rows(name: str, n: int, hi: int) -> dict:
    """Integer-valued rows rich in ties (the percentiles then fall on, or between, repeated values)."""
    rng = rng_of(name)
    return {"energy": rng.integers(0, hi, n).astype(np.float32), "pitch": rng.integers(-hi, hi, n).astype(np.float32),
            "f0": (rng.integers(0, 3, n) * 100).astype(np.float32)}


def fences_of(row: np.ndarray):
    """numpy's own percentile and the reference's fence arithmetic (src/tools/utils.py:142-150) on a float32 row."""
    p25, p75 = np.percentile(row, 25), np.percentile(row, 75)
    return p25, p75, p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)


def fence_rows(count: int = 6):
    """Integer rows in which a value EQUALS a fence exactly (the strict comparison drops it), searched on the CPU: the first ``count``
    seeds whose row has such a value at the lower fence, the upper fence, or both, with a positive interquartile range."""
    out, seed = [], 0
    while len(out) < count:
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        seed += 1
        n = int(rng.integers(6, 40))
        row = rng.integers(0, 12, n).astype(np.float32)
        row[int(rng.integers(0, n))] += float(rng.integers(8, 30))
        row[int(rng.integers(0, n))] -= float(rng.integers(8, 30))
        p25, p75, lower, upper = fences_of(row)
        if p75 > p25 and ((row == lower).any() or (row == upper).any()):
            out.append(row)
    assert len(out) >= 4
    return out


def _with(row_e, row_p, name):
    rng = rng_of(name)
    return {"energy": row_e, "pitch": row_p, "f0": f0_row(rng, len(row_e))}


def corpora() -> dict:
    """name -> list of utterances."""
    c = {}
    c["lengths"] = [utterance(f"len{n}", n) for n in LENGTHS]
    mix = ((1, 64, 9, 257, 3, 128, 1025), (65, 2, 1023, 7, 129, 4, 63), (255, 5, 8, 127, CAP, 2, 9))
    for i, lens in enumerate(mix):
        c[f"ragged{i}"] = [utterance(f"ragged{i}/{j}", n) for j, n in enumerate(lens)]
    c["ties"] = [integer_rows(f"ties{j}", n, hi) for j, (n, hi) in enumerate(((5, 3), (8, 2), (64, 4), (65, 6), (129, 3), (257, 10), (1025, 5)))]
    c["outliers"] = [heavy_outliers(f"out{j}", n) for j, n in enumerate((9, 63, 128, 257, 1023, 40, 20))]
    fr = fence_rows()
    c["fences"] = [_with(r, r[::-1].copy() - np.float32(3.0), f"fence{j}") for j, r in enumerate(fr)]
    # [0, 5, 5, 10]: the fences are 0 and 10 exactly, the kept values are the two 5s: zero variance, std 1.  A constant row and a row of
    # one frame keep nothing.
    q = np.array([0, 5, 5, 10], np.float32)
    c["constant"] = [_with(q, q + np.float32(2.0), "const0"), _with(np.full(17, 3.5, np.float32), np.full(17, -2.0, np.float32), "const1"),
                     _with(np.array([7.25], np.float32), np.array([1.5], np.float32), "const2"), _with(q[::-1].copy(), q + np.float32(2.0), "const3")]
    # all-unvoiced and all-voiced tracks beside mixed ones
    c["voicing"] = [utterance("v0", 40, "unvoiced"), utterance("v1", 33, "voiced"), utterance("v2", 65, "mixed"), utterance("v3", 5, "unvoiced"),
                    utterance("v4", 129, "mixed")]
    c["twelve"] = [utterance(f"twelve{j}", n) for j, n in enumerate((31, 64, 200, 7, 513, 90, 1, 128, 77, 300, 2, 1000))]
    return c


def batch(utts, key: str, poison: bool = True):
    """The utterances' rows of one kind as a padded batch -> (values [B, T] float32, lens [B] int64); the padding is NaN."""
    lens = np.array([len(u[key]) for u in utts], np.int64)
    x = np.full((len(utts), int(lens.max())), np.nan if poison else 0.0, np.float32)
    for b, u in enumerate(utts):
        x[b, :lens[b]] = u[key]
    return x, lens


def digest(utts) -> np.ndarray:
    h = hashlib.sha256()
    for u in utts:
        for k in ("energy", "pitch", "f0"):
            h.update(np.ascontiguousarray(u[k], dtype="<f4").tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def load() -> dict:
    """The fixture: name -> array."""
    with np.load(GOLD) as g:
        return {k: g[k] for k in g.files}
