"""CPU tests of bench.py's command line and of ``--dump-outputs``' writer (the GPU run itself: tests/test_gpu_bench_dump.py)."""
import os

import numpy as np
import pytest

import bench


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_steps_and_warmup_are_checked():
    a = bench.parse(["--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "out"
    assert bench.parse([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_small_outputs_are_written_whole_as_float32_or_float64(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"loss": np.float64(141.0625), "u_loc_unconstrained": rng.standard_normal((3, 5)).astype(np.float32),
              "_kernel.variance_unconstrained": rng.standard_normal(1), "counts": np.arange(6, dtype=np.int32).reshape(2, 3)}
    written = bench.dump_outputs(str(tmp_path), arrays)
    got = _files(tmp_path)
    assert set(got) == set(arrays) and written == {k: int(np.asarray(v).size) for k, v in arrays.items()}
    for k, v in arrays.items():
        v = np.asarray(v)
        assert got[k].dtype == (np.float32 if v.dtype == np.float32 else np.float64), k
        assert got[k].shape == v.shape and np.array_equal(got[k], v), k


def test_large_outputs_are_sampled_within_the_budget_the_same_way_every_time(tmp_path):
    big = np.arange(200_000, dtype=np.float64).reshape(400, 500)          # the values name their own flat index
    arrays = {"loss": np.float64(1.5), "small": np.ones(10, dtype=np.float32), "big": big, "big32": big.astype(np.float32)}
    budget = 256 * 1024
    runs = []
    for i in range(2):
        d = tmp_path / str(i)
        bench.dump_outputs(str(d), arrays, budget=budget)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= budget
        runs.append(_files(d))
    a, b = runs
    assert a.keys() == b.keys() == arrays.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["small"], arrays["small"]) and float(a["loss"]) == 1.5
    for k in ("big", "big32"):
        s = a[k].astype(np.float64)
        assert s.ndim == 1 and 1000 < s.size < big.size, (k, s.size)
        assert (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < big.size and np.array_equal(s, np.round(s)), k


def test_full_is_off_by_default():
    assert bench.parse([]).full is False
    assert bench.parse(["--full", "--steps", "3"]).full is True
