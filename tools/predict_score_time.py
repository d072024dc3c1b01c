"""Time and peak memory of the per-row log predictive densities (SparseMultinomialGDRF.pointwise_log_likelihood, csrc/predict_score.h)
beside the summed score that was there before it and the torch composition a user had for the rows.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 10 topics, S = 64 Philox samples, D = 2:
dense counts at V = 50 (about 60 % of a row's words present) and V = 4096 (1 %), CSR counts at V = 16384 (1 %).  On the first vocabulary
two yardsticks run beside it: predictive_perplexity - the one existing kernel that does the same sums, keeps one number and throws the
rows away (its code is the same in this tree and its parent, so alternating with it in one process IS the parent alternated with the
branch) - and the composition sample_topic_probs (S x N x K stored) -> `@ word_topic_matrix` -> log -> the statistics with torch in row
pieces, where its S x piece x V intermediate fits.  The calls take turns round by round in one process, so that clock and thermal drift
hit all alike.  One call = the whole model method (input scaling, factorisation, forward, the sample kernel), timed with HIP events
after warm-up; the peak is torch's allocator peak over the call, above what was allocated before it.  Prints the median and spread of
each point, the largest difference between the two ways, then one JSON line.

    python tools/predict_score_time.py [--rows 100000] [--topics 10] [--samples 64] [--dense 50 4096] [--csr 16384] [--compose-up-to 50]
                                       [--reps 10] [--warmup 3]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.data import mark_checked  # noqa: E402
from gdrf_amd.kernels import RBF  # noqa: E402
from gdrf_amd.models import SparseMultinomialGDRF  # noqa: E402

PIECE = 16384          # rows of the composition's S x piece x V intermediate: 210 MB in float32 at S = 64, V = 50


def make_model(K, V, seed=0):
    """a model with a contracted posterior (as after training), so that f_var is neither 0 nor the prior's"""
    model = SparseMultinomialGDRF(world=[(0.0, 1.0)] * 2, kernel=RBF(input_dim=2, lengthscale=torch.tensor(0.07), variance=torch.tensor(25.0)),
                                  num_observation_categories=V, num_topic_categories=K, dirichlet_param=0.01, n_points=[16, 16],
                                  fixed_inducing_points=True, inducing_init="grid", maxjitter=15, jitter=1e-6, device="cuda:0",
                                  dtype=torch.float32, seed=7)
    e, g, M = model._engine, torch.Generator().manual_seed(seed), 256
    e.view("u_loc").copy_(0.3 * torch.randn(K, M, generator=g))
    e.view("phi_unc").copy_(torch.randn(K, V, generator=g))
    e.view("u_scale_tril_unc").copy_((0.01 * torch.randn(M, M, generator=g)).tril(-1).expand(K, M, M) - 1.5 * torch.eye(M))
    return model


def csr_counts(N, V, density, g):
    """(N, V) CSR counts on the device with round(V density) stored entries a row: one column drawn from each of that many equal strides
    of the vocabulary, so a row's columns are distinct and ascending by construction"""
    nnz = max(1, round(V * density))
    stride = V // nnz
    col = (torch.arange(nnz, device="cuda") * stride)[None] + torch.randint(0, stride, (N, nnz), generator=g, device="cuda")
    val = torch.randint(1, 7, (N * nnz,), generator=g, device="cuda", dtype=torch.int32)
    crow = torch.arange(N + 1, device="cuda", dtype=torch.int64) * nnz
    return mark_checked(torch.sparse_csr_tensor(crow, col.reshape(-1), val, size=(N, V)))


def dense_counts(N, V, density, g):
    ws = torch.randint(1, 7, (N, V), generator=g, device="cuda", dtype=torch.int32)
    ws[torch.rand(N, V, generator=g, device="cuda") >= density] = 0
    return ws


def compose(model, xs, ws, S, seed):
    """lpd, mean_log_lik and var_log_lik from stored samples with torch: theta (S, N, K) once, log p (S, piece, V) piece by piece"""
    theta = model.sample_topic_probs(xs, S, seed=seed)
    phi = model.word_topic_matrix.to(theta)
    parts = []
    for a in range(0, xs.shape[0], PIECE):
        w = ws[a:a + PIECE]
        lp = (theta[:, a:a + PIECE] @ phi).log()
        parts.append(torch.where(w[None] != 0, w[None] * lp, torch.zeros_like(lp)).double().sum(-1))
    a_s = torch.cat(parts, dim=1)
    return dict(lpd=torch.logsumexp(a_s, 0) - math.log(S), mean_log_lik=a_s.mean(0), var_log_lik=a_s.var(0, unbiased=True))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--dense", type=int, nargs="*", default=[50, 4096], help="vocabularies scored from dense counts")
    ap.add_argument("--csr", type=int, nargs="*", default=[16384], help="vocabularies scored from CSR counts")
    ap.add_argument("--density", type=float, default=0.01, help="share of a row's words present, at V > 1000 (0.6 below)")
    ap.add_argument("--compose-up-to", type=int, default=50, help="the largest dense V at which the torch composition is run as well")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, K, S = a.rows, a.topics, a.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = torch.rand(N, 2, generator=g, device="cuda")
    calls, diffs = {}, {}
    for V, sparse in [(V, False) for V in a.dense] + [(V, True) for V in a.csr]:
        model = make_model(K, V)
        density = a.density if V > 1000 else 0.6
        ws = csr_counts(N, V, density, g) if sparse else dense_counts(N, V, density, g)
        tag = f"{'csr' if sparse else 'dense'}_V{V}"
        calls[f"pointwise_{tag}"] = lambda model=model, ws=ws: model.pointwise_log_likelihood(xs, ws, S, seed=1234)
        if not sparse and V <= a.compose_up_to:
            calls[f"summed_{tag}"] = lambda model=model, ws=ws: dict(ppl=model.predictive_perplexity(xs, ws, S, seed=1234))
            calls[f"composition_{tag}"] = lambda model=model, ws=ws: compose(model, xs, ws, S, 1234)
            got, want, one = calls[f"pointwise_{tag}"](), calls[f"composition_{tag}"](), calls[f"summed_{tag}"]()["ppl"]
            diffs[V] = {k: float((got[k] - want[k]).abs().max() / want[k].abs().max()) for k in want}
            diffs[V]["perplexity"] = abs(math.exp(-float(got["lpd"].sum()) / float(got["total"].sum())) - float(one)) / float(one)
            print(f"V={V}: largest difference (over the largest value) between pointwise_log_likelihood and the composition, and of the "
                  "perplexity from the rows to predictive_perplexity", {k: f"{v:.2e}" for k, v in diffs[V].items()}, flush=True)
    times, peaks = {k: [] for k in calls}, {k: 0 for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in out.values()), name
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - base)
            del out
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), peak_mb=peaks[name] / 2 ** 20)
        print(f"N={N} K={K} S={S} {name:24s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls, peak {res[name]['peak_mb']:.1f} MB", flush=True)
    print(json.dumps(dict(rows=N, M=256, K=K, S=S, reps=a.reps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          **{f"diff_V{V}_{k}": v for V, d in diffs.items() for k, v in d.items()})))


if __name__ == "__main__":
    main()
