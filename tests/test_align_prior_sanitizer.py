"""The generated prior's HIP-free half (e2e_tts_amd/csrc/align/prior_plan.h: argument checks, the beta-binomial parameters of a cell,
the column table's size and the index formulas) built with AddressSanitizer + UBSan on the CPU as a stand-alone program
(tests/csrc/align_prior_plan_test.cc, the pattern of tests/test_f0_sanitizer.py).  aligner.hip includes the same header on its host
and its device side, so these are the formulas the library ships."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "csrc", "align_prior_plan_test.cc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "align_prior_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f"sanitizer report, failed check or crash (rc={r.returncode}):\n{r.stderr[-3000:]}"
    return r.stdout.strip()


def test_the_kernels_walk_stays_inside_the_planned_tables(harness):
    """The column kernel's and the prior kernel's threads over ragged and padded batches: every index inside a heap table of exactly the
    planned size, every cell written exactly once, zeros where the definition has them, rows summing to less than 1."""
    assert run(harness, "walk").startswith("OK ")


def test_argument_checks(harness):
    assert run(harness, "checks") == "OK"


def test_the_formula_in_the_kernels_order_gives_the_host_paths_values(harness):
    """The three terms in aligner.hip's order of operations, with the C library's lgamma: within an fp32 ulp of scipy's pmf."""
    from e2e_tts_amd import aligner as al
    for P, M, s, t, k in [(7, 33, 1.0, 0, 0), (12, 70, 1.0, 35, 6), (40, 300, 2.5, 299, 39), (40, 300, 0.5, 10, 0), (33, 4000, 1.0, 2000, 16)]:
        want = np.float32(al.beta_binomial_prior_distribution(P, M, s)[t, k])
        got = np.float32(float(run(harness, "value", P, M, s, t, k)))
        assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1, (P, M, s, t, k, got, want)
    assert run(harness, "value", 7, 3, 0.0, 0, 0) == "ERR" and run(harness, "value", 7, 3, 1.0, 3, 0) == "ERR"
