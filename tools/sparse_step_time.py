"""Step time of the sparse row form (a torch.sparse_csr count matrix) against the dense vocabulary-streamed form on the same counts.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 20 topics, D = 2; synthetic counts with a
fixed number of stored entries per row (density x V, distinct columns).  The two forms take turns step by step in one process, so that
clock and thermal drift hit both alike.  One step = loss_and_grads + the Adam update, timed with HIP events after warm-up.  --sparse-only
times shapes whose dense counts do not fit (rows vocabulary entries-per-row triples).  Prints the median and spread of each point, then
one JSON line.

    python tools/sparse_step_time.py [--rows 100000] [--steps 20] [--warmup 5] [--vocab 4096 16384] [--density 0.01 0.05 0.25]
                                     [--sparse-only 1000000 16384 100]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.data import mark_checked  # noqa: E402
from tools.vocab_step_time import make_engine  # noqa: E402


def csr_counts(N, V, per, seed=2):
    """(N, V) CSR counts with `per` entries in every row: one column drawn from each of `per` equal bands of the vocabulary"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    band = V // per
    col = torch.randint(0, band, (N, per), generator=g, device="cuda") + torch.arange(per, device="cuda") * band
    val = torch.randint(1, 3, (N, per), generator=g, device="cuda", dtype=torch.int32)
    ws = torch.sparse_csr_tensor(torch.arange(0, N * per + 1, per, device="cuda"), col.reshape(-1), val.reshape(-1), size=(N, V))
    return mark_checked(ws)            # built well formed: skip the index check's host read


def time_point(N, K, V, per, Z, xs, steps, warmup, dense=True):
    wc = csr_counts(N, V, per)
    data = {"sparse": wc}
    if dense:
        data["streamed"] = wc.to_dense()
    engs = {f: make_engine("streamed" if f == "streamed" else "auto", N, K, V, Z) for f in data}
    times = {f: [] for f in data}
    for step in range(warmup + steps):
        for f, e in engs.items():
            eps = e.fill_eps(1234, step, 0, N)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.loss_and_grads(xs, data[f], eps)
            e.adam("adamw", 1e-3)
            t1.record()
            loss = e.read_out()["loss"]                   # synchronises, as a training loop reading the loss does
            if step >= warmup:
                times[f].append(t0.elapsed_time(t1))
            assert loss == loss, f"{f}: NaN loss at step {step}"
    del engs, data, wc
    torch.cuda.empty_cache()
    out = {}
    for f, t in times.items():
        out[f] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"N={N:8d} V={V:6d} entries/row={per:5d} {f:9s}: median {out[f]['median_ms']:.3f} ms  (min {out[f]['min_ms']:.3f}, "
              f"max {out[f]['max_ms']:.3f}) over {len(t)} steps", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--vocab", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--density", type=float, nargs="*", default=[0.01, 0.05, 0.25])
    ap.add_argument("--sparse-only", type=int, nargs="*", default=[], help="rows vocabulary entries-per-row, repeated: timed in the sparse form alone")
    a = ap.parse_args()
    K = a.topics
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 16, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    res = {}
    if a.vocab and a.density:
        xs = torch.rand(a.rows, 2, generator=torch.Generator().manual_seed(1)).cuda()
        for V in a.vocab:
            for d in a.density:
                per = max(1, int(round(d * V)))
                r = time_point(a.rows, K, V, per, Z, xs, a.steps, a.warmup)
                for f, q in r.items():
                    res[f"V{V}_d{d}_{f}"] = q
                print(f"V={V:6d} density {d}: sparse / streamed = {r['sparse']['median_ms'] / r['streamed']['median_ms']:.4f}", flush=True)
    for i in range(0, len(a.sparse_only) - 2, 3):
        N, V, per = a.sparse_only[i:i + 3]
        xs = torch.rand(N, 2, generator=torch.Generator().manual_seed(1)).cuda()
        res[f"N{N}_V{V}_e{per}_sparse"] = time_point(N, K, V, per, Z, xs, a.steps, a.warmup, dense=False)["sparse"]
    print(json.dumps(dict(rows=a.rows, M=Z.shape[0], K=K, steps=a.steps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})))


if __name__ == "__main__":
    main()
