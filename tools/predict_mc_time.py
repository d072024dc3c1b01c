"""Time of the Monte-Carlo predictive calls (Engine.predict_mc, csrc/predict_mc.h) beside the plug-in calls on the same rows.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 20 topics, V = 50 words, D = 2.  Modes 1
(moments of theta) and 2 (predictive score) at S = 64 and 256 Philox samples; gdrf_predict mode 4 (f_loc, f_var: the forward the
Monte-Carlo calls start with) and mode 3 (the plug-in perplexity sums).  The calls take turns round by round in one process, so that
clock and thermal drift hit all alike.  One call = the whole Engine method (factorisation, forward, the sample kernel), timed with HIP
events after warm-up, no host read inside the timed span beyond the call's own.  Prints the median and spread of each point, then one
JSON line.

    python tools/predict_mc_time.py [--rows 100000] [--topics 20] [--vocab 50] [--reps 20] [--warmup 5] [--samples 64 256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.vocab_step_time import make_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--vocab", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="*", default=[64, 256])
    a = ap.parse_args()
    N, K, V = a.rows, a.topics, a.vocab
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 16, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    e = make_engine("auto", N, K, V, Z)
    xs = torch.rand(N, 2, generator=torch.Generator().manual_seed(1)).cuda()
    ws = torch.randint(0, 3, (N, V), generator=torch.Generator(device="cuda").manual_seed(2), device="cuda", dtype=torch.int32)
    calls = {"predict_mode4": lambda: e.predict(xs, 4), "predict_mode3": lambda: e.predict(xs, 3, ws)}
    for S in a.samples:
        calls[f"mc_moments_S{S}"] = lambda S=S: e.predict_mc(xs, 1, S, seed=1234)
        calls[f"mc_score_S{S}"] = lambda S=S: e.predict_mc(xs, 2, S, ws=ws, seed=1234)
    times = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            assert bool(torch.isfinite(out).all()), name
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"N={N} K={K} V={V} {name:18s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls", flush=True)
    print(json.dumps(dict(rows=N, M=Z.shape[0], K=K, V=V, reps=a.reps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})))


if __name__ == "__main__":
    main()
