"""The statistics library's HIP-free half (e2e_tts_amd/csrc/stats/plan.h: argument checks, caps, the percentiles' virtual indices, the
workgroup and keys-per-thread choice, LDS bytes, the bitonic stage schedule, the key transform) built with AddressSanitizer + UBSan on
the CPU as a stand-alone program (tests/csrc/stats_plan_test.cc, the pattern of tests/test_f0_sanitizer.py).  stats.hip includes the
same header on its host and its device side, so these are the formulas the library ships."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "stats_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "stats_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_virtual_indices_against_int128(harness):
    """lo, hi and gamma for q = 25 and 75 at every n from 1 to 70 000 against (n - 1) q / 100 in __int128 and in double."""
    assert run(harness, "vindex") == "OK"


def test_schedule_sorts_every_permutation_of_up_to_8(harness):
    """The stage schedule on the scalar model of the kernel: every permutation of 1 to 8 distinct keys, and of 1 to 8 keys with ties."""
    out = run(harness, "perm")
    assert out.startswith("OK ") and int(out.split()[1]) > 46000


def test_schedule_sorts_random_rows_up_to_the_cap(harness):
    """Rows of every length class's edges (a power of two and that +- 1, the cap) and random lengths: register, shuffle and LDS stages
    index the keys a thread holds, lanes of its own wavefront, and an LDS image of exactly the planned size; the pad stays behind."""
    assert run(harness, "random").startswith("OK ")


def test_argument_checks_caps_and_keys(harness):
    assert run(harness, "checks") == "OK"
