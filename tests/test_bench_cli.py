"""bench.py's command line: --steps, ms_per_step, --full and --dump-outputs.

The helpers are checked on the host; one GPU test runs the benchmark itself
(that is what it is about) on a small --n-total and compares the dumped
outputs with the NumPy oracle's run from the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import REPO
from oracle import kmeans_oracle, synth

BENCH = os.path.join(REPO, "bench.py")


def test_sample_rows_is_fixed_and_bounded():
    assert bench.sample_rows(bench.DUMP_SAMPLE_VALUES) is None
    n = 100_000_000
    rows = bench.sample_rows(n)
    assert rows.dtype == np.int64 and 0 <= rows[0] and rows[-1] < n
    assert np.all(np.diff(rows) > 0)  # sorted, distinct
    assert 0.9 * bench.DUMP_SAMPLE_VALUES < rows.size <= bench.DUMP_SAMPLE_VALUES
    np.testing.assert_array_equal(rows, bench.sample_rows(n))
    # a wide output keeps fewer rows: the same number of values
    wide = bench.sample_rows(n, 6)
    assert wide.size <= bench.DUMP_SAMPLE_VALUES // 6


def test_sampled_keeps_small_outputs_whole():
    a = np.arange(12).reshape(6, 2)
    out = bench.sampled("counts", a)
    assert list(out) == ["counts"] and out["counts"] is a
    big = np.arange(bench.DUMP_SAMPLE_VALUES + 5, dtype=np.int32)
    out = bench.sampled("labels", big)
    assert sorted(out) == ["labels", "labels_rows"]
    np.testing.assert_array_equal(out["labels"], big[out["labels_rows"]])


def test_dump_outputs_writes_float64_npy(tmp_path):
    d = tmp_path / "sub" / "out"
    bench.dump_outputs(str(d), {"centroids": np.array([[0.1, 2.0 ** -24]]),
                                "labels": np.array([3, 0, 63], dtype=np.int64),
                                "max_ts_us": [1_762_000_000_000_001]})
    assert sorted(os.listdir(d)) == ["centroids.npy", "labels.npy", "max_ts_us.npy"]
    for name in os.listdir(d):
        assert np.load(d / name).dtype == np.float64
    np.testing.assert_array_equal(np.load(d / "centroids.npy"), [[0.1, 2.0 ** -24]])
    np.testing.assert_array_equal(np.load(d / "labels.npy"), [3, 0, 63])
    assert int(np.load(d / "max_ts_us.npy")[0]) == 1_762_000_000_000_001


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    a = np.zeros(bench.DUMP_MAX_BYTES // 8 + 1, dtype=np.int8)  # one value too many as float64
    with pytest.raises(RuntimeError, match="more than"):
        bench.dump_outputs(str(tmp_path / "out"), {"a": a})
    assert not (tmp_path / "out").exists()


def test_steps_below_one_is_an_error():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (no --full) on 50 000 points (seven seeding blocks, the
    last one partial): exactly --steps timed steps, no CPU baseline and no
    secondary legs, and the dumped centroids and labels are bit-identical to
    the oracle's after warmup + steps Lloyd iterations from the same seeds."""
    n, d, k, warmup, steps = 50_000, 16, 64, 1, 3
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--n-total", str(n), "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "point-iters/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n * 1e3 / out["ms_per_step"], rel=1e-9)
    assert "cpu_baseline" not in out and "secondary" not in out and out["seed_warm_s"] is None

    X = synth.generate(n, 0, n, d, k, 0x5EED)
    C0 = kmeans_oracle.kmeans_plusplus_init(X, k, random_state=42)
    np.random.seed(0)
    C, labels, _, taken = kmeans_oracle.lloyd(X, C0, warmup + steps, -1.0)
    assert taken == warmup + steps
    assert sorted(os.listdir(tmp_path / "o")) == ["centroids.npy", "labels.npy"]
    got_C, got_l = np.load(tmp_path / "o" / "centroids.npy"), np.load(tmp_path / "o" / "labels.npy")
    assert got_C.dtype == np.float64 and got_l.dtype == np.float64
    np.testing.assert_array_equal(got_l, labels)
    np.testing.assert_array_equal(got_C, C)
