"""The critic library's HIP-free half (e2e_tts_amd/csrc/critic/plan.h: argument checks, length formulas, the stride fold, the rows every
launch covers, workspace sizes and the pass cap, the grouped kernel's shape support, tile choice and LDS image) built with
AddressSanitizer + UBSan on the CPU as a stand-alone program (tests/csrc/critic_plan_test.cc, the pattern of
tests/test_compare_sanitizer.py).  critic.hip includes the same header on its host and its device side, so these are the formulas the
library ships."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "critic_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "critic_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_geometry_sweep(harness):
    """Rows of 12 to 700 samples and a few long ones (up to 2^24) through the default and the quarter tables: every launch's rows hold
    every sequence and what the next dense layer's fold reads, the folded convolution on buffers of exactly the planned sizes equals the
    strided one, and the grouped kernel's staging and fragment reads stay inside the planned LDS image, every word read having been
    written, for the planned tile and forced ones."""
    assert run(harness, "sweep").startswith("OK ")


def test_score_lengths_of_the_default_tables(harness):
    """What torch produced for n = 2049: MPD scores of 26 / 27 / 30 / 28 / 33 and MSD scores of 33 / 17 / 9."""
    assert run(harness, "lens", 2049) == "26 27 30 28 33 33 17 9"
    assert run(harness, "lens", 12) == "2 3 5 7 11 1 1 1"


def test_argument_checks_and_refusals_by_name(harness):
    assert run(harness, "checks") == "OK"


def test_rows_per_pass_under_the_cap(harness):
    assert run(harness, "cap") == "OK"
