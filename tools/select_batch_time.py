"""Time of the batch choice (Engine.select_batch; csrc/select_batch.h) beside gdrf_predict mode 4 on the same rows.

float32 arrays with the f64 solve, M = 256 inducing points (16 x 16 grid), K = 10 topics, D = 2.  Cases: N = 1e5 with count 8 and 64, N = 4096
with count 64.  One call = the whole Engine method (factorisation of K_uu, forward, W in the solve precision, count picks), timed with HIP
events after warm-up; mode 4 (f_loc, f_var) is the forward that the call contains.  The calls take turns round by round in one process, so
that clock and thermal drift hit all alike.  The time per pick is (select_batch - mode 4) / count; beside it stands the time the bytes of
a pick - N M elements of W and, on average, N K (count - 1) / 2 of the factor columns, 8 bytes each - take at 8 TB/s, and their ratio.

At N = 4096 the torch composition runs too: predict_cov (the K dense covariances) and the same recursion in torch on the device; its time
and the largest difference of its gains from select_batch's, relative to the first gain, are printed.  Then one JSON line.

    python tools/select_batch_time.py [--reps 10] [--warmup 3] [--noise 0.1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.vocab_step_time import make_engine  # noqa: E402

HBM_BYTES_PER_S = 8e12


def torch_composition(e, xs, count, s2):
    """the recursion of csrc/select_batch.h in float64 torch on the K dense covariances of predict_cov"""
    C = e.predict_cov(xs, 0).double()                                  # (K, n, n)
    K, n = C.shape[0], C.shape[1]
    d = C.diagonal(dim1=1, dim2=2).clone()
    cols = torch.zeros(K, count, n, dtype=torch.float64, device=C.device)
    taken = torch.zeros(n, dtype=torch.bool, device=C.device)
    idx, gains = [], []
    for t in range(count):
        g = 0.5 * torch.log1p(d.clamp_min(0.0) / s2).sum(0)
        g = torch.where(taken, torch.full_like(g, -1.0), g)
        p = torch.argmax(g)
        idx.append(p)
        gains.append(g[p])
        taken[p] = True
        c = (C[:, :, p] - torch.einsum("ksn,ks->kn", cols[:, :t], cols[:, :t, p])) / (d[:, p] + s2).sqrt()[:, None]
        cols[:, t] = c
        d = d - c * c
    return torch.stack(idx), torch.stack(gains)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--topics", type=int, default=10)
    a = ap.parse_args()
    K, V, s2 = a.topics, 8, a.noise
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 16, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    M = Z.shape[0]
    cases = [(100000, 8), (100000, 64), (4096, 64)]
    nmax = max(n for n, _ in cases)
    e = make_engine("auto", nmax, K, V, Z)
    xall = torch.rand(nmax, 2, generator=torch.Generator().manual_seed(1)).cuda()
    calls = {}
    for n in sorted({n for n, _ in cases}):
        calls[f"n{n}_predict_mode4"] = lambda xs=xall[:n].contiguous(): e.predict(xs, 4)
    for n, c in cases:
        calls[f"n{n}_select_batch_c{c}"] = lambda xs=xall[:n].contiguous(), c=c: e.select_batch(xs, c, s2)[1]
    calls["n4096_torch_composition_c64"] = lambda xs=xall[:4096].contiguous(): torch_composition(e, xs, 64, s2)[1]
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
        print(f"M={M} K={K} {name:30s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, max {res[name]['max_ms']:.3f}) "
              f"over {len(t)} calls", flush=True)
    out = dict(M=M, K=K, noise=s2, reps=a.reps)
    for n, c in cases:
        per_pick = (res[f"n{n}_select_batch_c{c}"]["median_ms"] - res[f"n{n}_predict_mode4"]["median_ms"]) / c
        floor = (n * M + n * K * (c - 1) / 2) * 8 / HBM_BYTES_PER_S * 1e3
        print(f"n={n} count={c}: {per_pick * 1e3:.1f} us per pick; its bytes at 8 TB/s take {floor * 1e3:.1f} us: ratio {per_pick / floor:.2f}", flush=True)
        out[f"n{n}_c{c}_per_pick_us"], out[f"n{n}_c{c}_floor_us"] = per_pick * 1e3, floor * 1e3
    xs = xall[:4096].contiguous()
    idx, gains = e.select_batch(xs, 64, s2)
    tidx, tgains = torch_composition(e, xs, 64, s2)
    diff = float((gains - tgains).abs().max() / gains[0])
    same = int((idx == tidx).sum())
    print(f"n=4096 count=64: largest difference of the gains from the torch composition on predict_cov's float32 covariances {diff:.3e} "
          f"of the first gain; {same} of 64 picks equal", flush=True)
    out.update(torch_gain_diff=diff, torch_equal_picks=same, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
