"""The conditioning library's HIP-free half (e2e_tts_amd/csrc/condition/plan.h: positions, argument checks, capacities, tile choice, the
scalar window test and range walk) built with AddressSanitizer + UBSan on the CPU as a stand-alone program
(tests/csrc/condition_plan_test.cc, the pattern of tests/test_resample_sanitizer.py).  condition.hip includes the same header on its host
and its device side, so these are the formulas the library ships."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "condition_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "condition_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_sweep_against_the_scalar_walk(harness):
    """Six rates x lengths of 1 .. 3 s (whole ms, one sample more, an overhanging tail) x W 100 and 7 x the chosen tile and forced tiles
    of 64, 128 and 448 starts: bins by bin_of, the window test tile by tile in an exactly-sized prefix buffer, the walk word by word with
    room for every range and with room for one (capacity overflow: the true count is kept, nothing is written past cap), and the kept span
    of the three trim modes, all against the definition evaluated directly on the samples."""
    assert run(harness, "sweep").startswith("OK ")


def test_int64_positions(harness):
    """pos and bin_of against __int128 up to 2^30 ms and 384 kHz; len_ms rounds half to even."""
    assert run(harness, "big") == "OK"


def test_argument_checks(harness):
    assert run(harness, "checks") == "OK"


def test_tile_choice(harness):
    assert run(harness, "tile", 100) == "T=512 lds_words=612"
    assert run(harness, "tile", 1) == "T=256 lds_words=257"
    assert run(harness, "tile", 4096) == "T=3584 lds_words=7680"
