"""The pitch library's HIP-free half (e2e_tts_amd/csrc/f0/plan.h: argument checks, window and lag formulas, the frame grid in int64
sample positions, tile choice and LDS plan) built with AddressSanitizer + UBSan on the CPU as a stand-alone program
(tests/csrc/f0_plan_test.cc, the pattern of tests/test_resample_sanitizer.py).  f0.hip includes the same header on its host and its
device side, so these are the formulas the library ships."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "f0_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "f0_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_small_geometry_sweep(harness):
    """Small rates, four floors, six hops, rows from empty to a few tiles: the staged samples, every wavefront's window with its zero
    tail, its row of lags and its candidate list are indexed inside an LDS image of exactly the planned size, the staged windows are
    the definition's, and the padded lag sums equal the definition's."""
    assert run(harness, "sweep").startswith("OK ")


def test_int64_positions(harness):
    """n = 2^31 and beyond, up to the 2^32 limit: frame counts, centres and first samples against __int128; the frame and cell caps."""
    assert run(harness, "big") == "OK"


def test_argument_checks(harness):
    assert run(harness, "checks") == "OK"


def test_tile_choice(harness):
    """The geometries the project serves: window, lag range, frames a tile, LDS bytes.  64 KiB is never exceeded; 48 kHz with floor 80
    (W = 1801) is served with four frames a tile, floor 40 there is refused."""
    assert run(harness, "tile", 22050, 256, 80, 750) == "W=827 tau=[30,275] lags=277 AL=1112 F=16 stage=4667 lds_bytes=40944"
    assert run(harness, "tile", 16000, 128, 80, 750) == "W=601 tau=[22,200] lags=202 AL=812 F=16 stage=2521 lds_bytes=26352"
    assert run(harness, "tile", 48000, 512, 80, 750) == "W=1801 tau=[64,600] lags=602 AL=2412 F=4 stage=3337 lds_bytes=61616"
    assert run(harness, "tile", 48000, 512, 40, 750).startswith("ERR") and run(harness, "tile", 22050, 256, 80, 30000).startswith("ERR")
