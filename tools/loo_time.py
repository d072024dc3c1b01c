"""Time and peak memory of PSIS leave-one-out (SparseMultinomialGDRF.pointwise_loo, csrc/predict_loo.h) beside pointwise_log_likelihood,
whose work it does once before the ordering and the fit, the PSIS stage alone (SparseMultinomialGDRF.psis on a stored matrix) and the
torch composition a user had.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 10 topics, D = 2, the model and the counts of
tools/predict_score_time.py: dense counts at V = 50 (about 60 % of a row's words present) and V = 4096 (1 %), CSR counts at V = 16384
(1 %), each at S = 64 and S = 256 Philox samples; pointwise_log_likelihood runs beside every S = 64 point.  The stage alone runs on the
(S, N) matrix pointwise_loo returned.  The composition - sample_topic_probs (S x N x K stored) -> `@ word_topic_matrix` -> log -> the
(S, N) log likelihoods in row pieces -> the float64 restatement of tests/_loo_ref.py (torch.sort and a batched fit, whose (m, M, N)
intermediate is the peak) on the device - runs where it fits, at the smallest vocabulary.  The calls take turns round by round in one
process, so that clock and thermal drift hit all alike.  One call = the whole model method, timed with HIP events after warm-up; the peak
is torch's allocator peak over the call, above what was allocated before it.  Prints the median and spread of each point, the largest
difference between pointwise_loo and the composition, then one JSON line.

    python tools/loo_time.py [--rows 100000] [--topics 10] [--samples 64 256] [--dense 50 4096] [--csr 16384] [--compose-up-to 50]
                             [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from predict_score_time import PIECE, csr_counts, dense_counts, make_model  # noqa: E402
from tests._loo_ref import psis as psis_restated  # noqa: E402


def compose(model, xs, ws, S, seed):
    """elpd_loo, pareto_k and ess from stored samples with torch: theta (S, N, K) once, log p (S, piece, V) piece by piece, the PSIS
    restatement on the (S, N) matrix"""
    theta = model.sample_topic_probs(xs, S, seed=seed)
    phi = model.word_topic_matrix.to(theta)
    parts = []
    for a in range(0, xs.shape[0], PIECE):
        w = ws[a:a + PIECE]
        lp = (theta[:, a:a + PIECE] @ phi).log()
        parts.append(torch.where(w[None] != 0, w[None] * lp, torch.zeros_like(lp)).double().sum(-1))
    return dict(zip(("elpd_loo", "pareto_k", "ess"), psis_restated(torch.cat(parts, dim=1))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--samples", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--dense", type=int, nargs="*", default=[50, 4096], help="vocabularies scored from dense counts")
    ap.add_argument("--csr", type=int, nargs="*", default=[16384], help="vocabularies scored from CSR counts")
    ap.add_argument("--density", type=float, default=0.01, help="share of a row's words present, at V > 1000 (0.6 below)")
    ap.add_argument("--compose-up-to", type=int, default=50, help="the largest dense V at which the torch composition is run as well")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, K = a.rows, a.topics
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = torch.rand(N, 2, generator=g, device="cuda")
    calls, diffs, plans = {}, {}, {}
    for V, sparse in [(V, False) for V in a.dense] + [(V, True) for V in a.csr]:
        model = make_model(K, V)
        density = a.density if V > 1000 else 0.6
        ws = csr_counts(N, V, density, g) if sparse else dense_counts(N, V, density, g)
        for S in a.samples:
            tag = f"{'csr' if sparse else 'dense'}_V{V}_S{S}"
            calls[f"loo_{tag}"] = lambda model=model, ws=ws, S=S: model.pointwise_loo(xs, ws, S, seed=1234)
            if S == min(a.samples):
                calls[f"pointwise_{tag}"] = lambda model=model, ws=ws, S=S: model.pointwise_log_likelihood(xs, ws, S, seed=1234)
            got = model.pointwise_loo(xs, ws, S, seed=1234, return_log_lik=True)
            plans[tag] = model._engine.last_loo_plan()
            if not sparse and V == min(a.dense):
                log_lik = got["log_lik"]
                calls[f"stage_S{S}"] = lambda model=model, log_lik=log_lik: model.psis(log_lik)
                if V <= a.compose_up_to and S == min(a.samples):
                    calls[f"composition_{tag}"] = lambda model=model, ws=ws, S=S: compose(model, xs, ws, S, 1234)
                    want = calls[f"composition_{tag}"]()
                    fitted = ~torch.isnan(want["pareto_k"]) & ~torch.isnan(got["pareto_k"])
                    diffs[tag] = dict(elpd_loo=float((got["elpd_loo"] - want["elpd_loo"]).abs().max() / want["elpd_loo"].abs().max()),
                                      pareto_k=float((got["pareto_k"] - want["pareto_k"])[fitted].abs().max()),
                                      ess=float(((got["ess"] - want["ess"]).abs() / want["ess"]).max()))
                    print(f"{tag}: largest difference between pointwise_loo and the composition (elpd_loo over the largest value, pareto_k "
                          "absolute, ess relative; the composition's log likelihoods are float32 sums of another order)",
                          {k: f"{v:.2e}" for k, v in diffs[tag].items()}, flush=True)
            k = got["pareto_k"]
            print(f"{tag}: plan {plans[tag]}, rows not fitted {int(torch.isnan(k).sum())}, pareto_k > 0.7 {int((k > 0.7).sum())}, "
                  f"median pareto_k {float(k[~torch.isnan(k)].median()):.3f}, median ess {float(got['ess'].median()):.1f}", flush=True)
            del got
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
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - base)
            del out
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), peak_mb=peaks[name] / 2 ** 20)
        print(f"N={N} K={K} {name:28s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls, peak {res[name]['peak_mb']:.1f} MB", flush=True)
    print(json.dumps(dict(rows=N, M=256, K=K, reps=a.reps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          **{f"diff_{t}_{k}": v for t, d in diffs.items() for k, v in d.items()},
                          **{f"plan_{t}_{k}": v for t, d in plans.items() for k, v in d.items()})))


if __name__ == "__main__":
    main()
