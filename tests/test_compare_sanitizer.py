"""The comparison library's HIP-free half (e2e_tts_amd/csrc/compare/plan.h: argument checks, caps, the band predicate, the back-pointer
word and bit index, workspace sizes, tile and LDS plans) built with AddressSanitizer + UBSan on the CPU as a stand-alone program
(tests/csrc/compare_plan_test.cc, the pattern of tests/test_f0_sanitizer.py).  compare.hip includes the same header on its host and
its device side, so these are the formulas the library ships."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "compare_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "compare_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_geometry_sweep(harness):
    """Lengths from 1 to 600 on both sides (and 1100 x 1100: two chunks of 1024 rows), workgroups of 64 to 1024 threads, no band and
    bands 0, 1, 2 and 8: the search kernel's chunks and diagonals index the two
    exchange rows, the handed-on row and the back-pointer words inside buffers of exactly the planned sizes, no two cells share their
    two bits, the chunked sweep gives the plain DP's total, the back-track stays inside the planned path and sums to that total, and
    every band >= 1 holds a path.  The cepstra kernel's basis and tile rows are indexed inside its planned LDS image."""
    assert run(harness, "sweep").startswith("OK ")


def test_caps_against_int128(harness):
    """The band predicate (and its symmetry) and the back-pointer word index at the frame cap and the band cap against __int128; a whole
    batch's offsets at the caps; the packed path cell at the largest indices."""
    assert run(harness, "caps") == "OK"


def test_argument_checks(harness):
    assert run(harness, "checks") == "OK"


def test_lds_plans_stay_under_64_kib(harness):
    """The plans the project serves, and the refusal of one that does not fit."""
    assert run(harness, "lds", 80, 13) == "stride=84 tile=64 cepstra_lds_bytes=25872 search_lds_bytes=49152 walk_lds_bytes=32764"
    assert run(harness, "lds", 20, 64) == "stride=28 tile=64 cepstra_lds_bytes=14336 search_lds_bytes=49152 walk_lds_bytes=32764"
    out = run(harness, "lds", 128, 64)
    assert out.startswith("stride=132 tile=") and int(out.split("cepstra_lds_bytes=")[1].split()[0]) <= 65536
    assert run(harness, "lds", 1024, 64).startswith("ERR") and run(harness, "lds", 80, 65).startswith("ERR")
