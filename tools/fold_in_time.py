"""Time of the fold-in calls (Engine.fold_in, csrc/foldin.h) beside the plug-in calls on the same rows.

float32 arrays with the f64 solve, N = 1e6 rows, M = 256 inducing points (16 x 16 grid), K = 10 topics, V = 50 words, D = 2, about 1000
counts per row drawn from softmax(m + s eps) Phi with (m, s) the model's own prior of the row.  gdrf_predict mode 4 (f_loc, f_var: the
forward a fold-in call starts with) and mode 3 (the plug-in perplexity sums); fold-in theta at 64 iterations with tol = 0 (every row runs
all of them) and with tol = 1e-6 (rows stop as they converge), dense and CSR; the completion score.  The calls take turns round by round in
one process, so that clock and thermal drift hit all alike.  One call = the whole Engine method (factorisation, forward, the fold-in
kernel), timed with HIP events after warm-up, no host read inside the timed span beyond the call's own.  Prints the median and spread of
each point and the iterations the rows used, then one JSON line.

    python tools/fold_in_time.py [--rows 1000000] [--topics 10] [--vocab 50] [--iters 64] [--counts 1000] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.data import to_csr  # noqa: E402
from tools.vocab_step_time import make_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=50)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--counts", type=float, default=1000.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, K, V, T = a.rows, a.topics, a.vocab, a.iters
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 16, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    e = make_engine("auto", N, K, V, Z)
    xs = torch.rand(N, 2, generator=torch.Generator().manual_seed(1)).cuda()
    g = torch.Generator(device="cuda").manual_seed(2)
    lv = e.predict(xs, 4)
    mu = lv[0] + (lv[1] + e.view("log_noise").exp()) * torch.randn(K, N, generator=g, device="cuda")
    p = torch.softmax(mu, 0).T @ torch.softmax(e.view("phi_unc"), -1)
    ws = torch.poisson(a.counts * p, generator=g).to(torch.int32).contiguous()          # Poisson(R p_v) words: a Multinomial of Poisson(R) draws
    del lv, mu, p
    half = (ws // 2).contiguous()
    rest = (ws - half).contiguous()
    ws_csr = to_csr(ws)
    calls = {"predict_mode4": lambda: e.predict(xs, 4), "predict_mode3": lambda: e.predict(xs, 3, ws),
             f"fold_in_theta_T{T}_tol0": lambda: e.fold_in(xs, ws, 0, T, 0.0),
             f"fold_in_theta_T{T}_tol1e-6": lambda: e.fold_in(xs, ws, 0, T, 1e-6),
             f"fold_in_theta_T{T}_tol1e-6_csr": lambda: e.fold_in(xs, ws_csr, 0, T, 1e-6),
             f"fold_in_score_T{T}_tol1e-6": lambda: e.fold_in(xs, half, 3, T, 1e-6, ws_score=rest)}
    times, used = {k: [] for k in calls}, {}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            if isinstance(out, tuple):
                out, diag = out
                used[name] = (float(diag[2].mean()), float(diag[2].max()), float(diag[1].max()))
            assert bool(torch.isfinite(out).all()), name
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        it = "" if name not in used else f"  iterations used mean {used[name][0]:.1f} max {used[name][1]:.0f}, largest |g|/R {used[name][2]:.1e}"
        print(f"N={N} K={K} V={V} {name:32s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls{it}", flush=True)
    print(json.dumps(dict(rows=N, M=Z.shape[0], K=K, V=V, iters=T, counts=a.counts, reps=a.reps, nnz=int(ws_csr.values().numel()),
                          **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})))


if __name__ == "__main__":
    main()
