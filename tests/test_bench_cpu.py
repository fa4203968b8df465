"""
CPU: the output dump of bench.py (`--dump-outputs DIR`): what it writes, in which types, within its size limit, and the
fixed sample it takes of outputs larger than that.
"""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _written(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def test_dump_outputs_types_and_values(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"field": rng.normal(size=1000), "small_ids": rng.integers(0, 2 ** 24, 500),
              "large_ids": np.array([0, 2 ** 24, 5], dtype=np.int64), "empty": np.zeros(0, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path), arrays)
    got = _written(tmp_path)
    assert sorted(got) == sorted(arrays)
    assert got["field"].dtype == np.float64 and np.array_equal(got["field"], arrays["field"])
    # integers: float32 only where every value is exact in it
    assert got["small_ids"].dtype == np.float32 and np.array_equal(got["small_ids"].astype(np.int64), arrays["small_ids"])
    assert got["large_ids"].dtype == np.float64 and np.array_equal(got["large_ids"].astype(np.int64), arrays["large_ids"])
    assert got["empty"].size == 0


def test_dump_outputs_fixed_sample_within_limit(tmp_path):
    rng = np.random.default_rng(4)
    arrays = {"field": rng.normal(size=200_000), "ids": rng.integers(0, 1000, 300_000)}
    limit = 400_000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=limit)
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= limit
    a, b = _written(tmp_path / "a"), _written(tmp_path / "b")
    for name, full in arrays.items():
        assert 0 < a[name].size < full.size
        assert np.array_equal(a[name], b[name])  # the same positions from run to run
        pos = np.sort(np.random.default_rng(0).choice(full.size, a[name].size, replace=False))  # (as the docstring states)
        assert np.array_equal(a[name], full[pos].astype(a[name].dtype))


def test_dump_outputs_refused_off_the_one_gpu_line(tmp_path):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path)],
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode == 2 and "--dump-outputs" in proc.stderr
