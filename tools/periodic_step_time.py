"""Step time of a Periodic context on one input axis against an RBF-ARD context on two (the same embedded width), alternated in one
process.

N = 1e6 rows, M = 512 inducing points, K = 10 topics, V = 50 words, float32 arrays with the f64 solve (the defaults of
gdrf_amd.Engine).  Periodic: D = 1, period 1, lengthscale 0.02, inducing points evenly spaced over one period.  RBF-ARD: D = 2, a 32 x 16 grid.  One step = loss_and_grads + the Adam update, timed with HIP events after warm-up; the two contexts
take turns step by step so that clock and thermal drift hit both alike.  Prints the median and the spread (min, max) of each and
the ratio of the medians, then one JSON line.

    python tools/periodic_step_time.py [--rows 1000000] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import Engine  # noqa: E402


def make_engine(periodic, N, K, V, Z, seed=0):
    if periodic:
        e = Engine(N, Z.shape[0], K, V, 1, dtype=torch.float32, kernel="periodic", jitter=1e-6, process_group=None)
    else:
        e = Engine(N, Z.shape[0], K, V, 2, dtype=torch.float32, kernel="rbf", jitter=1e-6, process_group=None, ard=True)
    e.set_inducing_points(Z)
    e.set_dirichlet(torch.full((K, V), 0.01, dtype=torch.float64))
    g = torch.Generator().manual_seed(seed)
    M = Z.shape[0]
    e.view("log_variance").fill_(float(torch.tensor(25.0).log()))
    e.view("u_loc").copy_(0.3 * torch.randn(K, M, generator=g))
    e.view("phi_unc").copy_(torch.randn(K, V, generator=g))
    e.view("u_scale_tril_unc").copy_((0.01 * torch.randn(M, M, generator=g)).tril(-1).expand(K, M, M) - 1.5 * torch.eye(M))
    if periodic:
        e.view("log_lengthscale").fill_(float(torch.tensor(0.02).log()))
        e.view("log_period").fill_(0.0)
    else:
        e.view("log_lengthscale").copy_(torch.tensor([0.05, 0.1]).log())
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    N, K, V = a.rows, 10, 50
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 32, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z2 = torch.stack([gx.flatten(), gy.flatten()], 1)
    Z1 = (torch.arange(512, dtype=torch.float64) / 512)[:, None]       # one period, no point twice on the circle
    g = torch.Generator().manual_seed(1)
    xs2 = torch.rand(N, 2, generator=g).cuda()
    xs1 = xs2[:, :1].contiguous()
    ws = torch.randint(0, 3, (N, V), generator=g, dtype=torch.int32).cuda()
    engs = {"ard": make_engine(False, N, K, V, Z2), "periodic": make_engine(True, N, K, V, Z1)}
    rows = {"ard": xs2, "periodic": xs1}
    times = {k: [] for k in engs}
    for step in range(a.warmup + a.steps):
        for name, e in engs.items():
            eps = e.fill_eps(1234, step, 0, N)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.loss_and_grads(rows[name], ws, eps)
            e.adam("adamw", 1e-3)
            t1.record()
            loss = e.read_out()["loss"]                   # synchronises, as a training loop reading the loss does
            if step >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
            assert loss == loss, f"{name}: NaN loss at step {step}"
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"{name}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, max {res[name]['max_ms']:.3f}) over {len(t)} steps")
    ratio = res["periodic"]["median_ms"] / res["ard"]["median_ms"]
    print(f"periodic / ard: {ratio:.4f}")
    print(json.dumps(dict(rows=N, M=Z2.shape[0], K=K, V=V, steps=a.steps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          ratio=ratio)))


if __name__ == "__main__":
    main()
