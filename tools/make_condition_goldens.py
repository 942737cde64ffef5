#!/usr/bin/env python3
"""Records tests/golden/condition_cases.npz: what the standard library's audioop gives for every row of tests/condition_cases.py, through
the pydub layer as the issue restates it (ms positions, zero-padded slices, seek_step 1, range merging).  Inputs are regenerated from
seeds, so the file holds results only: per row the silence ranges, and per trim mode the kept span, its audioop.rms, its sum of squares,
the loudness gain and the sha256 of audioop.mul's bytes; for stereo rows the sha256 of audioop.tomono's bytes.

    python tools/make_condition_goldens.py          # needs audioop (Python < 3.13)"""
import audioop
import hashlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import condition_cases as cc  # noqa: E402

W, THRESH_DB = 100, -50


def sha(b: bytes):
    return np.frombuffer(hashlib.sha256(b).digest(), np.uint8).copy()


def seg(x, a, b):
    """pydub's slice by sample positions: the bytes of x[a:b], zero-padded to b - a samples"""
    s = x[a:b].tobytes()
    return s + b"\0" * (2 * (b - a) - len(s))


def detect_silence(x, rate):
    """pydub.silence.detect_silence(min_silence_len=100, silence_thresh=-50, seek_step=1) on audioop.rms"""
    pos = lambda p: int(p * (rate / 1000.0))   # noqa: E731  (pydub's _parse_position)
    L = round(1000 * (len(x) / rate))
    if L < W:
        return [], L
    thresh = 10 ** (THRESH_DB / 20) * 32768
    starts = [i for i in range(L - W + 1) if audioop.rms(seg(x, pos(i), pos(i + W)), 2) <= thresh]
    if not starts:
        return [], L
    ranges, prev, cur = [], starts[0], starts[0]
    for i in starts[1:]:
        if i > prev + W:   # pydub: not continuous and a silence gap
            ranges.append([cur, prev + W])
            cur = i
        prev = i
    ranges.append([cur, prev + W])
    return ranges, L


def record(out, key, x, rate):
    pos = lambda p: int(p * (rate / 1000.0))   # noqa: E731
    ranges, L = detect_silence(x, rate)
    out[f"{key}/ranges"] = np.array(ranges, np.int32).reshape(-1, 2)
    out[f"{key}/len_ms"] = np.int64(L)
    for trim in ("none", "reference", "both"):
        if not ranges or trim == "none":
            s, e, kept = 0, L, x.tobytes()
        else:
            s = ranges[0][1] if ranges[0][0] == 0 else 0
            e = L
            if trim == "both" and ranges[-1][1] == L:
                e = ranges[-1][0]
            kept = seg(x, pos(s), pos(e)) if e > s else b""
        n = len(kept) // 2
        r = audioop.rms(kept, 2) if n else 0
        S = sum(int(v) ** 2 for v in np.frombuffer(kept, np.int16))
        assert r == (math.isqrt(S // n) if n else 0)
        gain = 10 ** ((cc.TARGET_DBFS - 20 * math.log(r / 32768, 10)) / 20) if r else 1.0
        out[f"{key}/{trim}/span"] = np.array([s, e, n], np.int64)
        out[f"{key}/{trim}/rms"] = np.int64(r)
        out[f"{key}/{trim}/sumsq"] = np.uint64(S)
        out[f"{key}/{trim}/gain"] = np.float64(gain)
        out[f"{key}/{trim}/mul_sha"] = sha(audioop.mul(kept, 2, gain))
        out[f"{key}/{trim}/mul1_sha"] = sha(audioop.mul(kept, 2, 1.0))


def main():
    out = {}
    for name, case in cc.cases().items():
        for b, row in enumerate(case["rows"]):
            key = f"{name}/{b}"
            if case["channels"] == 2:
                mono = np.frombuffer(audioop.tomono(row.tobytes(), 2, 0.5, 0.5), np.int16)
                out[f"{key}/tomono_sha"] = sha(mono.tobytes())
            else:
                mono = row
            record(out, key, mono, case["rate"])
            print(key, "N", len(mono), "ranges", out[f"{key}/ranges"].tolist(), "ref span", out[f"{key}/reference/span"].tolist(), "both span",
                  out[f"{key}/both/span"].tolist())
    path = os.path.join(ROOT, "tests", "golden", "condition_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
