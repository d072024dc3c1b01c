"""Step time of SVI.step with no mean, a plain-callable mean and a trainable torch.nn.Module mean at the headline shape, alternated in
one process.

N = 1e6 rows, M = 512 inducing points (32 x 16 grid), K = 10 topics, V = 50 words, D = 2, float32 arrays (the defaults of
SparseMultinomialGDRF).  Three models with the same data and initial parameters:
  none      mean_function=None;
  callable  a (K, n) linear trend as a plain callable: its values are data to the step;
  module    the same trend as an nn.Module with (K, D+1) trainable weights: the step also reads the row adjoints back, reduces them
            through the module by autograd and trains the weights.
One step = svi.step(xs, ws), which returns the loss and so synchronises; timed by the wall clock after warm-up, the models taking
turns step by step so that clock and thermal drift hit all three alike.  Prints the median and spread of each and the ratios to
"none", then one JSON line.

    python tools/mean_step_time.py [--rows 1000000] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd import poutine  # noqa: E402
from gdrf_amd.infer import SVI, Trace_ELBO  # noqa: E402
from gdrf_amd.kernels import RBF  # noqa: E402
from gdrf_amd.models import SparseMultinomialGDRF  # noqa: E402
from gdrf_amd.optim import Adam  # noqa: E402


class Trend(torch.nn.Module):
    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(w.clone())

    def forward(self, x):
        return self.w[:, :-1] @ x.T + self.w[:, -1:]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    N, K, V, dev = a.rows, 10, 50, "cuda:0"
    g = torch.Generator().manual_seed(1)
    xs = torch.rand(N, 2, generator=g).to(dev)
    ws = torch.randint(0, 3, (N, V), generator=g, dtype=torch.int32).to(dev)
    w = (0.5 * torch.randn(K, 3, generator=g)).to(dev)
    means = {"none": None, "callable": lambda x, w=w: w[:, :-1] @ x.T + w[:, -1:], "module": Trend(w).to(dev)}
    runs = {}
    for name, mf in means.items():
        model = SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2, kernel=RBF(input_dim=2, lengthscale=0.07, variance=torch.tensor(25.0)),
                                      num_observation_categories=V, num_topic_categories=K, dirichlet_param=0.01, n_points=[32, 16],
                                      fixed_inducing_points=True, inducing_init="grid", maxjitter=15, jitter=1e-6, device=dev, seed=7,
                                      mean_function=mf)
        sc = poutine.scale(scale=1.0 / N)
        runs[name] = SVI(model=sc(model.model), guide=sc(model.guide), optim=Adam({"lr": 1e-3}), loss=Trace_ELBO())
    times = {k: [] for k in runs}
    for step in range(a.warmup + a.steps):
        for name, svi in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = svi.step(xs=xs, ws=ws, subsample=False)
            t1 = time.perf_counter()
            if step >= a.warmup:
                times[name].append(1e3 * (t1 - t0))
            assert loss == loss, f"{name}: NaN loss at step {step}"
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"{name}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, max {res[name]['max_ms']:.3f}) over {len(t)} steps")
    ratios = {f"{k}_over_none": res[k]["median_ms"] / res["none"]["median_ms"] for k in ("callable", "module")}
    for k, r in ratios.items():
        print(f"{k}: {r:.4f}")
    moved = float((runs["module"].gdrf._mean_function.w.detach() - w).abs().max())
    print(json.dumps(dict(rows=N, M=512, K=K, V=V, steps=a.steps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          **ratios, module_weights_moved=moved)))


if __name__ == "__main__":
    main()
