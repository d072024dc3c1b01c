"""Step time of the separable spatiotemporal product RBF(x, y) x Periodic(t) against Periodic on two axes and RBF-ARD on three, alternated
in one process.  The product and Periodic D = 2 run on 4 embedded coordinates, RBF-ARD D = 3 on 3.

N = 1e6 rows, M = 512 inducing points, K = 10 topics, V = 50 words, float32 arrays with the f64 solve (the defaults of
gdrf_amd.Engine).  Product: D = 3, RBF-ARD on (x, y) with lengthscales (0.05, 0.1), Periodic on t with lengthscale 0.5 and period 0.25.
Periodic: D = 2, lengthscale 0.05, period 1.  RBF-ARD: D = 3, lengthscales (0.05, 0.1, 0.2).  Inducing points: an 8 x 8 x 8 grid for
the three-axis contexts, a 32 x 16 grid for Periodic.  One step =
loss_and_grads + the Adam update, timed with HIP events after warm-up; the contexts take turns step by step so that clock and thermal
drift hit them alike.  Prints the median and the spread (min, max) of each and the ratios of the medians, then one JSON line.

    python tools/product_step_time.py [--rows 1000000] [--steps 20] [--warmup 5] [--only product|periodic|ard]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import Engine  # noqa: E402

PRODUCT = [dict(name="kern0", kind="rbf", active_dims=[0, 1], lengthscales=2, periods=0),
           dict(name="kern1", kind="periodic", active_dims=[2], lengthscales=1, periods=1)]


def make_engine(kind, N, K, V, Z, seed=0):
    D = Z.shape[1]
    if kind == "product":
        e = Engine(N, Z.shape[0], K, V, D, dtype=torch.float32, kernel="product", product=PRODUCT, jitter=1e-6, process_group=None)
    elif kind == "periodic":
        e = Engine(N, Z.shape[0], K, V, D, dtype=torch.float32, kernel="periodic", jitter=1e-6, process_group=None)
    else:
        e = Engine(N, Z.shape[0], K, V, D, dtype=torch.float32, kernel="rbf", jitter=1e-6, process_group=None, ard=True)
    e.set_inducing_points(Z)
    e.set_dirichlet(torch.full((K, V), 0.01, dtype=torch.float64))
    g = torch.Generator().manual_seed(seed)
    M = Z.shape[0]
    e.view("u_loc").copy_(0.3 * torch.randn(K, M, generator=g))
    e.view("phi_unc").copy_(torch.randn(K, V, generator=g))
    e.view("u_scale_tril_unc").copy_((0.01 * torch.randn(M, M, generator=g)).tril(-1).expand(K, M, M) - 1.5 * torch.eye(M))
    if kind == "product":
        e.view("kern0.log_variance").fill_(float(torch.tensor(25.0).log()))
        e.view("kern1.log_variance").fill_(0.0)
        e.view("kern0.log_lengthscale").copy_(torch.tensor([0.05, 0.1]).log())
        e.view("kern1.log_lengthscale").fill_(float(torch.tensor(0.5).log()))
        e.view("kern1.log_period").fill_(float(torch.tensor(0.25).log()))
    else:
        e.view("log_variance").fill_(float(torch.tensor(25.0).log()))
        if kind == "periodic":
            e.view("log_lengthscale").fill_(float(torch.tensor(0.05).log()))
            e.view("log_period").fill_(0.0)
        else:
            e.view("log_lengthscale").copy_(torch.tensor([0.05, 0.1, 0.2]).log())
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("product", "periodic", "ard"), default=None, help="time one context alone (e.g. under a profiler)")
    a = ap.parse_args()
    N, K, V = a.rows, 10, 50
    ax = torch.linspace(0, 1, 8, dtype=torch.float64)
    Z3 = torch.stack([c.flatten() for c in torch.meshgrid(ax, ax, ax, indexing="ij")], 1)
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 32, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z2 = torch.stack([gx.flatten(), gy.flatten()], 1)
    g = torch.Generator().manual_seed(1)
    xs3 = torch.rand(N, 3, generator=g).cuda()
    xs2 = xs3[:, :2].contiguous()
    ws = torch.randint(0, 3, (N, V), generator=g, dtype=torch.int32).cuda()
    Zs = {"product": Z3, "periodic": Z2, "ard": Z3}
    engs = {k: make_engine(k, N, K, V, Zs[k]) for k in Zs if a.only in (None, k)}
    rows = {"product": xs3, "periodic": xs2, "ard": xs3}
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
    ratios = {f"product_over_{k}": res["product"]["median_ms"] / res[k]["median_ms"] for k in ("periodic", "ard") if a.only is None}
    for k, r in ratios.items():
        print(f"{k}: {r:.4f}")
    print(json.dumps(dict(rows=N, M=Z3.shape[0], K=K, V=V, steps=a.steps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          **ratios)))


if __name__ == "__main__":
    main()
