"""Time of the posterior-predictive count sampler (Engine.sample_counts, csrc/sample_counts.h) beside the torch composition a user
would otherwise write on the same device.

float32 arrays, N = 1e5 rows, K = 10 topics, totals of 1000 tokens per row, at two shapes: V = 50 words with S = 16 samples, and
V = 4096 words with S = 4.  theta is a fixed (S, N, K) array of random proportions (drawing it is not what is timed).  Timed are mode 0
(the replicated counts), mode 1 (the check statistics, no replicate stored) and, per sample, ``torch.multinomial(theta_s Phi, T,
replacement=True)`` plus a ``scatter_add_`` of ones into the (N, V) count matrix.  The calls take turns round by round in one process,
so that clock and thermal drift hit all alike; each is timed with HIP events after warm-up.  Prints the median and spread of each
point, the rate in token draws per second, then one JSON line per shape.

    python tools/sample_counts_time.py [--rows 100000] [--topics 10] [--total 1000] [--reps 10] [--warmup 2] [--shapes 50:16 4096:4]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import Engine  # noqa: E402


def make_engine(K, V, seed=0):
    """a small context: the sampler reads Phi from the parameters and holds nothing per row"""
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 4, dtype=torch.float64), torch.linspace(0, 1, 4, dtype=torch.float64), indexing="ij")
    e = Engine(64, 16, K, V, 2, dtype=torch.float32, jitter=1e-6, process_group=None)
    e.set_inducing_points(torch.stack([gx.flatten(), gy.flatten()], 1))
    e.set_dirichlet(torch.full((K, V), 0.01, dtype=torch.float64))
    e.view("phi_unc").copy_(torch.randn(K, V, generator=torch.Generator().manual_seed(seed)))
    return e


def torch_counts(theta, phi, T):
    """the composition on the device: every token index is materialised, (N, T) int64 per sample"""
    S, N, _ = theta.shape
    out = torch.zeros(S, N, phi.shape[1], dtype=torch.int32, device=theta.device)
    ones = torch.ones(N, T, dtype=torch.int32, device=theta.device)
    for s in range(S):
        out[s].scatter_add_(1, torch.multinomial(theta[s] @ phi, T, replacement=True), ones)
    return out


def time_shape(N, K, V, S, T, reps, warmup):
    e = make_engine(K, V)
    g = torch.Generator(device="cuda").manual_seed(1)
    theta = torch.softmax(torch.randn(S, N, K, generator=g, device="cuda"), -1).contiguous()
    totals = torch.full((N,), T, dtype=torch.int32, device="cuda")
    ws = torch.randint(0, 3, (N, V), generator=g, device="cuda", dtype=torch.int32)
    phi = torch.softmax(e.view("phi_unc"), -1)
    calls = {"counts_mode0": lambda: e.sample_counts(theta, totals, seed=1234),
             "stats_mode1": lambda: e.sample_counts(theta, totals, 1, ws=ws, seed=1234)[0],
             "torch_multinomial": lambda: torch_counts(theta, phi, T)}
    times = {k: [] for k in calls}
    for rep in range(warmup + reps):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            if rep == 0 and name != "stats_mode1":
                assert int(out.sum()) == S * N * T, name
            del out
            if rep >= warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"N={N} K={K} V={V} S={S} T={T} {name:18s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls, {S * N * T / res[name]['median_ms'] / 1e6:.2f} G draws/s", flush=True)
    print(json.dumps(dict(rows=N, K=K, V=V, S=S, total=T, reps=reps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})), flush=True)
    del e, theta, ws
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--total", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=["50:16", "4096:4"], help="V:S pairs")
    a = ap.parse_args()
    for sh in a.shapes:
        V, S = (int(x) for x in sh.split(":"))
        time_shape(a.rows, a.topics, V, S, a.total, a.reps, a.warmup)


if __name__ == "__main__":
    main()
