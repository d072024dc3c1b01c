"""Step time of the LDS row forms (rows_form="auto") and the vocabulary-streamed form (rows_form="streamed") over the vocabulary size.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 20 topics, D = 2.  At V = 64 and 300
both forms run and take turns step by step, so that clock and thermal drift hit both alike; at V = 1000, 4096 and 16384 only the
streamed form runs (the LDS forms reject K x V that large).  One step = loss_and_grads + the Adam update, timed with HIP events after
warm-up.  Prints the median and spread of each (V, form), then one JSON line.

    python tools/vocab_step_time.py [--rows 100000] [--steps 20] [--warmup 5] [--shared 64 300] [--streamed-only 1000 4096 16384]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import Engine  # noqa: E402


def make_engine(rows_form, N, K, V, Z, seed=0):
    e = Engine(N, Z.shape[0], K, V, 2, dtype=torch.float32, jitter=1e-6, process_group=None, rows_form=rows_form)
    e.set_inducing_points(Z)
    e.set_dirichlet(torch.full((K, V), 0.01, dtype=torch.float64))
    g = torch.Generator().manual_seed(seed)
    M = Z.shape[0]
    e.view("log_variance").fill_(float(torch.tensor(25.0).log()))
    e.view("u_loc").copy_(0.3 * torch.randn(K, M, generator=g))
    e.view("phi_unc").copy_(torch.randn(K, V, generator=g))
    e.view("u_scale_tril_unc").copy_((0.01 * torch.randn(M, M, generator=g)).tril(-1).expand(K, M, M) - 1.5 * torch.eye(M))
    e.view("log_lengthscale").fill_(float(torch.tensor(0.1).log()))
    return e


def time_forms(forms, N, K, V, Z, xs, steps, warmup):
    g = torch.Generator(device="cuda").manual_seed(2)
    ws = torch.randint(0, 3, (N, V), generator=g, device="cuda", dtype=torch.int32)
    engs = {f: make_engine(f, N, K, V, Z) for f in forms}
    times = {f: [] for f in forms}
    for step in range(warmup + steps):
        for f, e in engs.items():
            eps = e.fill_eps(1234, step, 0, N)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.loss_and_grads(xs, ws, eps)
            e.adam("adamw", 1e-3)
            t1.record()
            loss = e.read_out()["loss"]                   # synchronises, as a training loop reading the loss does
            if step >= warmup:
                times[f].append(t0.elapsed_time(t1))
            assert loss == loss, f"{f}: NaN loss at step {step}"
    del engs, ws
    torch.cuda.empty_cache()
    out = {}
    for f, t in times.items():
        out[f] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"V={V:6d} {f:9s}: median {out[f]['median_ms']:.3f} ms  (min {out[f]['min_ms']:.3f}, max {out[f]['max_ms']:.3f}) over {len(t)} steps",
              flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shared", type=int, nargs="*", default=[64, 300], help="vocabulary sizes timed in both forms")
    ap.add_argument("--streamed-only", type=int, nargs="*", default=[1000, 4096, 16384], help="vocabulary sizes timed in the streamed form")
    a = ap.parse_args()
    N, K = a.rows, a.topics
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 16, dtype=torch.float64), torch.linspace(0, 1, 16, dtype=torch.float64), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    xs = torch.rand(N, 2, generator=torch.Generator().manual_seed(1)).cuda()
    res = {}
    for V in a.shared:
        for f, r in time_forms(("auto", "streamed"), N, K, V, Z, xs, a.steps, a.warmup).items():
            res[f"V{V}_{f}"] = r
        print(f"V={V:6d} streamed / auto: {res[f'V{V}_streamed']['median_ms'] / res[f'V{V}_auto']['median_ms']:.4f}", flush=True)
    for V in a.streamed_only:
        res[f"V{V}_streamed"] = time_forms(("streamed",), N, K, V, Z, xs, a.steps, a.warmup)["streamed"]
    print(json.dumps(dict(rows=N, M=Z.shape[0], K=K, steps=a.steps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})))


if __name__ == "__main__":
    main()
