"""Step time of an isotropic and an ARD (one lengthscale per input dimension) context at the headline shape, alternated in one process.

N = 1e6 rows, M = 512 inducing points (32 x 16 grid), K = 10 topics, V = 50 words, D = 2, float32 arrays with the f64 solve (the
defaults of gdrf_amd.Engine).  One step = loss_and_grads + the Adam update, timed with HIP events after warm-up; the two contexts
take turns step by step so that clock and thermal drift hit both alike.  Prints the median and the spread (min, max) of each and
the ratio of the medians, then one JSON line.

    python tools/ard_step_time.py [--rows 1000000] [--steps 20] [--warmup 5] [--kernel rbf]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import Engine  # noqa: E402


def make_engine(ard, N, K, V, kernel, Z, seed=0):
    e = Engine(N, Z.shape[0], K, V, 2, dtype=torch.float32, kernel=kernel, jitter=1e-6, process_group=None, ard=ard)
    e.set_inducing_points(Z)
    e.set_dirichlet(torch.full((K, V), 0.01, dtype=torch.float64))
    g = torch.Generator().manual_seed(seed)
    M = Z.shape[0]
    e.view("log_variance").fill_(float(torch.tensor(25.0).log()))
    e.view("u_loc").copy_(0.3 * torch.randn(K, M, generator=g))
    e.view("phi_unc").copy_(torch.randn(K, V, generator=g))
    e.view("u_scale_tril_unc").copy_((0.01 * torch.randn(M, M, generator=g)).tril(-1).expand(K, M, M) - 1.5 * torch.eye(M))
    ls = torch.tensor([0.05, 0.1]) if ard else torch.tensor(0.07)
    e.view("log_lengthscale").copy_(ls.log())
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel", default="rbf")
    a = ap.parse_args()
    N, K, V = a.rows, 10, 50
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 32, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    g = torch.Generator().manual_seed(1)
    xs = torch.rand(N, 2, generator=g).cuda()
    ws = torch.randint(0, 3, (N, V), generator=g, dtype=torch.int32).cuda()
    engs = {"iso": make_engine(False, N, K, V, a.kernel, Z), "ard": make_engine(True, N, K, V, a.kernel, Z)}
    times = {k: [] for k in engs}
    for step in range(a.warmup + a.steps):
        for name, e in engs.items():
            eps = e.fill_eps(1234, step, 0, N)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.loss_and_grads(xs, ws, eps)
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
    ratio = res["ard"]["median_ms"] / res["iso"]["median_ms"]
    print(f"ard / iso: {ratio:.4f}")
    print(json.dumps(dict(rows=N, M=Z.shape[0], K=K, V=V, kernel=a.kernel, steps=a.steps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          ratio=ratio)))


if __name__ == "__main__":
    main()
