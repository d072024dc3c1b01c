"""GPU: ``bench.py --dump-outputs`` writes what the last timed step returned, and the same arguments give the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--rows", "30000", "--n-points", "8", "8", "--cpu-baseline-n", "0", "--knm-iters", "2", "--kernel-pass-steps", "1"]


def _bench(out_dir, warmup, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", str(warmup), "--steps", str(steps),
                        "--dump-outputs", str(out_dir)] + SMALL, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    files = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), files


@pytest.mark.timeout(900)
def test_dump_outputs_holds_the_last_timed_step_and_repeats_exactly(tmp_path):
    d1, a = _bench(tmp_path / "a", 1, 2)
    _, b = _bench(tmp_path / "b", 1, 2)
    d3, c = _bench(tmp_path / "c", 2, 1)          # the same three steps, the last of them the only timed one
    assert d1["steps"] == 2 and d3["steps"] == 1 and abs(d1["value"] * d1["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert {"loss", "u_loc_unconstrained", "u_scale_tril_unconstrained", "_word_topic_matrix_map_unconstrained"} <= set(a)
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64 << 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), k
    assert float(a["loss"]) == d1["final_loss"]
    for other in (b, c):
        assert other.keys() == a.keys()
        for k in a:
            assert other[k].dtype == a[k].dtype and np.array_equal(other[k], a[k]), k


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_without_the_full_measurements():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--steps", "2",
                        "--rows", "30000", "--n-points", "8", "8"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 2
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3 and d["metric"].startswith("ELBO steps/sec")
    assert not {"roofline", "roofline_knm", "kernel_ms_per_step", "kernel_pass_steps", "perplexity", "cpu_baseline",
                "gpu_over_cpu"} & set(d)
