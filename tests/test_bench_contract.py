"""bench.py's output contract: ONE JSON line on stdout with the driver's keys, plus `roofline` (and `cpu_baseline` at N = 1) with
--full; a plain run times exactly --steps steps and nothing else, and --dump-outputs writes what its last step returned; without a GPU
it refuses to run instead of falling back to a CPU path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=600):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    r = run_bench("--steps", "1", "--warmup", "0", "--no-cpu-baseline")
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    r = run_bench("--steps", "2", "--warmup", "1", "--batch", "4", "--no-cpu-baseline", "--full")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["unit"] == "audio samples/s" and d["value"] > 22050 * 100          # the >= 100 x real-time target, even at B = 4
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s")
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0 < rf["frac"] < 1
    # value and ms_per_step describe the same timed region
    samples = 4 * 768 * 256
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


# what only --full measures: per-kernel figures, every other configuration, the CPU baseline
FULL_ONLY_KEYS = ("roofline", "cpu_baseline", "hbm_resident", "split_precision_mode", "fp32_mode", "latency_b1_ms", "parity", "c3_mixed",
                  "c4_sharded", "c5_longform")


def one_json_line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_pcm(tmp_path):
    """A plain run: exactly --steps timed steps, none of what --full adds, and --dump-outputs holds the PCM of the last timed step -- the
    headline batch is fixture bench_b32's, whose rows `sel` the reference pinned (within 1 LSB on >= 99.9 % of the strided samples)."""
    d = one_json_line(run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)))
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert [k for k in FULL_ONLY_KEYS if k in d] == []
    samples = 32 * 768 * 256
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    g = np.load(os.path.join(ROOT, "tests", "golden", "bench_b32.npz"), allow_pickle=False)
    pcm, mel_lens = np.load(tmp_path / "pcm.npy"), np.load(tmp_path / "mel_lens.npy")
    assert pcm.dtype == np.float32 and pcm.shape == (32, 768 * 256)
    np.testing.assert_array_equal(mel_lens, g["mel_lens"])
    sel, ws = g["sel"], int(g["wav_stride"])
    assert (np.abs(pcm[sel][:, ::ws] - g["pcm_strided_sel"].astype(np.float32)) <= 1).mean() >= 0.999


def test_plain_and_full_runs_on_the_stand_in_engine(tmp_path):
    """The same two contracts on CPU with the stand-in engine (E2ETTS_BENCH_STUB=1, computes nothing): the plain line carries none of
    what --full adds and the step count it was given, --dump-outputs writes the last step's PCM and mel lengths in float32, and --full
    brings the roofline and the config-4 record back."""
    env = dict(os.environ, E2ETTS_BENCH_STUB="1", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *a], cwd=ROOT, env=env,  # noqa: E731
                                    capture_output=True, text=True, timeout=600)
    d = one_json_line(run("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)))
    assert d["data"] == "stub" and d["steps"] == 3 and d["warmup"] == 1
    assert [k for k in FULL_ONLY_KEYS if k in d] == []
    assert abs(d["value"] - 32 * 768 * 256 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert sorted(os.listdir(tmp_path)) == ["mel_lens.npy", "pcm.npy"]
    pcm, mel_lens = np.load(tmp_path / "pcm.npy"), np.load(tmp_path / "mel_lens.npy")
    assert pcm.dtype == mel_lens.dtype == np.float32 and pcm.shape == (32, 768 * 256) and (mel_lens == 768).all()
    d = one_json_line(run("--steps", "2", "--warmup", "1", "--full"))
    assert d["steps"] == 2 and "roofline" in d and d["c4_sharded"]["utterances"] == 256


def test_dump_outputs_keeps_a_large_output_to_a_fixed_sample(tmp_path):
    """Over the budget the largest array is cut to a seeded sample of sorted flat indices, written beside it; the same in every run,
    the files at most 64 MB in all; integers beyond float32's exact range are written as float64."""
    sys.path.insert(0, ROOT)
    import bench
    big = np.random.default_rng(5).integers(-32768, 32768, size=(64, 300_000)).astype(np.int16)   # 76.8 MB as float32
    lens = np.arange(64, dtype=np.int64) * 100_000_000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"pcm": big, "lens": lens})
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["lens.npy", "pcm.npy", "pcm_sample_index.npy"]
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 * 10**6
    idx = np.load(a / "pcm_sample_index.npy")
    assert idx.dtype == np.float64 and idx.size > 1_000_000 and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(np.load(a / "pcm.npy"), big.reshape(-1)[idx.astype(np.int64)].astype(np.float32))
    assert np.load(a / "lens.npy").dtype == np.float64 and (np.load(a / "lens.npy") == lens).all()
    for f in os.listdir(a):
        np.testing.assert_array_equal(np.load(a / f), np.load(b / f))


def test_bench_helpers_without_a_gpu():
    """Host-only pieces of bench.py: the CPUs a process may really use (affinity mask / cgroup quota, not os.cpu_count()), BASELINE
    config 3's length list and config 4's utterance list (config 3's lengths x 8, the same on every rank)."""
    sys.path.insert(0, ROOT)
    import bench
    n, why = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1) and isinstance(why, str) and why
    lens = bench.mixed_lengths(32)
    assert lens.min() == 40 and lens.max() == 200 and int(lens.sum()) * 6 == 23040 and len(lens) == 32
    a, b = bench.c4_id_lists(256), bench.c4_id_lists(256)
    assert a == b and len(a) == 256 and sum(len(x) for x in a) * 6 == 8 * 23040
    assert sorted(len(x) for x in a[:32]) == sorted(lens.tolist())
    assert all(4 <= t <= 130 for x in a[:8] for t in x)
