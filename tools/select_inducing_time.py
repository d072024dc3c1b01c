"""Time of the greedy choice of inducing points (Engine.select_inducing; csrc/select_inducing.h) beside the torch composition of the same loop.

float32 arrays with the f64 solve, RBF at lengthscale 0.1 and variance 25, D = 2, count = 512 picks.  Cases: N = 1e5; N = 1e6 thinned to the
131072 rows floor(i N / 131072) that choose_inducing_points looks at by default; N = 1e6 not thinned.  One call = the whole Engine method
(allocation and release of its (count + 1) N solve-precision elements included), timed with HIP events after warm-up; the median of the
repeated calls is reported.  The pass's traffic is the read of the history, count (count - 1) / 2 x N elements of 8 bytes over the whole
call: beside the time stands that figure as a rate and as a share of 8 TB/s.

The torch composition is the same loop in float64 torch on the same device: one argmax (read back by the host), one gather and several (N,)
passes per pick, the (count, N) history in a tensor.  Its time, its peak memory and how its picks and pivots compare are printed.  Then
one JSON line.

    python tools/select_inducing_time.py [--reps 5] [--warmup 1] [--count 512] [--skip-large]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import Engine, thin_rows  # noqa: E402

HBM_BYTES_PER_S = 8e12
LS, VAR = 0.1, 25.0


def torch_composition(X, count, floor):
    """the loop of csrc/select_inducing.h in float64 torch: (picks, pivots, trace)"""
    X = X.double()
    n = X.shape[0]
    d = torch.full((n,), VAR, dtype=torch.float64, device=X.device)
    c = torch.zeros(count, n, dtype=torch.float64, device=X.device)
    taken = torch.zeros(n, dtype=torch.bool, device=X.device)
    neg = torch.full_like(d, -float("inf"))
    picks, pivots, trace = [], [], []
    for t in range(count):
        p = int(torch.argmax(torch.where(taken, neg, d)))
        taken[p] = True
        piv = d[p].clone()
        if float(piv) > floor:
            col = VAR * torch.exp(-0.5 * ((X - X[p]) ** 2).sum(1) / (LS * LS))
            ct = (col - c[:t].T @ c[:t, p]) / piv.sqrt()
            c[t] = ct
            d = d - ct * ct
        picks.append(p)
        pivots.append(piv)
        trace.append(d.sum())
    return torch.tensor(picks, device=X.device), torch.stack(pivots), torch.stack(trace)


def timed(fn, reps, warmup):
    ts = []
    for rep in range(warmup + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        if rep >= warmup:
            ts.append(t0.elapsed_time(t1))
    return out, dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--skip-large", action="store_true", help="leave out N = 1e6 not thinned (4 GB of history, 8 GB in the torch composition)")
    a = ap.parse_args()
    T = a.count
    floor = max(1e-8, T * torch.finfo(torch.float64).eps * VAR)
    big = torch.rand(10 ** 6, 2, generator=torch.Generator().manual_seed(1))
    cases = {"n1e5": big[:10 ** 5], "n1e6_thinned": big[thin_rows(10 ** 6, 131072)]}
    if not a.skip_large:
        cases["n1e6"] = big
    out = dict(count=T, reps=a.reps, floor=floor)
    for name, xs in cases.items():
        n = xs.shape[0]
        eng = Engine(n, 16, 1, 2, 2, dtype=torch.float32, kernel="rbf", process_group=None)
        eng.view("log_lengthscale").fill_(math.log(LS))
        eng.view("log_variance").fill_(math.log(VAR))
        xd = xs.cuda().contiguous()
        (idx, piv, tr, rank), t_dev = timed(lambda: eng.select_inducing(xd, T, floor=floor), a.reps, a.warmup)
        hist = T * (T - 1) / 2 * n * 8
        rate = hist / (t_dev["median_ms"] * 1e-3)
        print(f"{name}: N={n} count={T} select_inducing median {t_dev['median_ms']:.2f} ms (min {t_dev['min_ms']:.2f}, max {t_dev['max_ms']:.2f}) over "
              f"{a.reps} calls; {t_dev['median_ms'] / T * 1e3:.1f} us per pick; history {hist / 1e9:.1f} GB -> {rate / 1e12:.2f} TB/s, "
              f"{100 * rate / HBM_BYTES_PER_S:.0f} % of 8 TB/s; buffers {(T + 1) * n * 8 / 1e9:.2f} GB held for the call; rank {rank}, "
              f"trace / (n var) {float(tr[-1]) / (n * VAR):.3e}", flush=True)
        del eng
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        (tidx, tpiv, ttr), t_torch = timed(lambda: torch_composition(xd, T, floor), max(1, a.reps // 2), a.warmup)
        peak = torch.cuda.max_memory_allocated() - base
        same = int((idx == tidx).sum())
        first = next((i for i in range(T) if int(idx[i]) != int(tidx[i])), T)
        dpiv = float((piv[:first + 1] - tpiv[:first + 1]).abs().max() / VAR)
        print(f"{name}: torch composition median {t_torch['median_ms']:.2f} ms, peak memory {peak / 1e9:.2f} GB: {t_torch['median_ms'] / t_dev['median_ms']:.1f} x "
              f"the device call; {same} of {T} picks equal (the first {first} all), pivots up to the first difference within {dpiv:.2e} of the variance",
              flush=True)
        out[name] = dict(n=n, device=t_dev, torch=t_torch, history_bytes=hist, rate_tb_s=rate / 1e12, torch_peak_bytes=peak, equal_picks=same,
                         first_difference=first, rank=rank)
        del tidx, tpiv, ttr, idx, piv, tr, xd
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
