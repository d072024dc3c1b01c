"""Time of the joint-posterior calls (Engine.predict_cov, Engine.sample_joint; csrc/predict_cov.h) beside gdrf_predict mode 4 on the same rows.

float32 arrays with the f64 solve, M = 512 inducing points (32 x 16 grid), K = 10 topics, D = 2; n = 1024, 2048 and the row cap
JOINT_MAX_ROWS.  predict_cov forms the K full covariances (K, n, n); sample_joint draws S = 64 Philox samples, its n x n Cholesky
factorisation in one workgroup included; mode 4 (f_loc, f_var) is the forward that each of the two contains.  The calls take turns round
by round in one process, so that clock and thermal drift hit all alike.  One call = the whole Engine method (factorisation of K_uu,
forward, products, for sample_joint the read of the failure flag), timed with HIP events after warm-up.  Prints the median and spread
of each point and the device memory in use at the largest size, then one JSON line.

    python tools/joint_time.py [--rows 1024 2048 4096] [--topics 10] [--samples 64] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import JOINT_MAX_ROWS  # noqa: E402
from tools.vocab_step_time import make_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, nargs="*", default=[1024, 2048, JOINT_MAX_ROWS])
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    K, S, V = a.topics, a.samples, 8
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 32, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    e = make_engine("auto", max(a.rows), K, V, Z)
    xall = torch.rand(max(a.rows), 2, generator=torch.Generator().manual_seed(1)).cuda()
    calls = {}
    for n in a.rows:
        xs = xall[:n].contiguous()
        calls[f"n{n}_predict_mode4"] = lambda xs=xs: e.predict(xs, 4)
        calls[f"n{n}_predict_cov"] = lambda xs=xs: e.predict_cov(xs, 0)
        calls[f"n{n}_sample_joint_S{S}"] = lambda xs=xs: e.sample_joint(xs, S, seed=1234)
    times = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            assert bool(torch.isfinite(out).all()), name
            del out
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"M={Z.shape[0]} K={K} {name:26s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls", flush=True)
    free, total = torch.cuda.mem_get_info()
    peak = torch.cuda.max_memory_allocated()
    print(f"joint jitter level of the last sample_joint: {e.last_joint_level}; device memory in use {(total - free) / 2 ** 20:.0f} MiB "
          f"(torch peak {peak / 2 ** 20:.0f} MiB of it)", flush=True)
    print(json.dumps(dict(M=Z.shape[0], K=K, S=S, reps=a.reps, joint_level=e.last_joint_level, used_mib=(total - free) / 2 ** 20,
                          **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})))


if __name__ == "__main__":
    main()
