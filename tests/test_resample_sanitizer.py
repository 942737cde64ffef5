"""The resampler's HIP-free half (e2e_tts_amd/csrc/resample/plan.h: argument checks, index formulas, coefficient table, stream
bookkeeping, tile choice) built with AddressSanitizer + UBSan on the CPU as a stand-alone program (tests/csrc/resample_plan_test.cc, the
pattern of tests/test_host_sanitizer.py).  resample.hip includes the same header on its host and its device side, so these are the
formulas the library ships."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "resample_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "resample_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_exhaustive_small_sweep(harness):
    """Every coprime (L, M) up to 6, every odd n_taps up to 15, lengths 1 .. 23, the chosen tile and forced tiles of 1 .. 8 L outputs, eight
    chunkings each: the table, the window, the LDS image and the stream's history are indexed inside exactly-sized heap buffers, and every
    launch reproduces the definition."""
    assert run(harness, "sweep").startswith("OK ")


def test_int64_positions(harness):
    """n = 2^31 and beyond, up to the 2^40 limit: centres, k_lo / k_hi, the outputs that exist and the history against __int128."""
    assert run(harness, "big") == "OK"


def test_argument_checks(harness):
    assert run(harness, "checks") == "OK"


def test_tile_choice(harness):
    """The ratios the project serves (default design): lanes per phase, repeats, LDS image.  64 KiB is never exceeded; an even M gets the
    padded image (shift > 0) that keeps the stride of a phase's lanes odd."""
    assert run(harness, "tile", 160, 441, 14113) == "S=32 nrep=1 shift=0 window=14201 lds=14201 outputs=5120 P=89 half=7056"
    assert run(harness, "tile", 320, 147, 10241) == "S=64 nrep=1 shift=0 window=9441 lds=9441 outputs=20480 P=33 half=5120"
    assert run(harness, "tile", 147, 320, 10241) == "S=32 nrep=1 shift=6 window=10310 lds=10471 outputs=4704 P=70 half=5120"
    assert run(harness, "tile", 1, 6, 193) == "S=64 nrep=27 shift=1 window=10561 lds=15841 outputs=1728 P=193 half=96"
    assert run(harness, "tile", 2, 1, 65) == "S=64 nrep=16 shift=0 window=1057 lds=1057 outputs=2048 P=33 half=32"
    assert run(harness, "tile", 2, 4, 65).startswith("ERR") and run(harness, "tile", 2, 1, 64).startswith("ERR")
