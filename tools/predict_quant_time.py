"""Time and peak memory of the credible-interval, exceedance and dominant-topic maps (SparseMultinomialGDRF.topic_probs_quantiles,
exceedance, dominant_topic_probs, word_probs_quantiles; csrc/predict_quant.h) beside the torch composition a user had before them.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 10 topics, S = 256 Philox samples, D = 2,
V = 50 words.  The composition is sample_topic_probs (S x N x K stored), then torch.sort along the samples and the type-7 interpolation,
`>` and a mean, argmax and a count.  A second model at V = 4096 times the word quantiles of 16 chosen words (the composition would
store S x N x 16 more values behind the S x N x K ones; it is not run).  topic_probs_mc - the forward plus one generation of the S draws
and their softmax - is the yardstick that says what the draws alone cost.  The calls take turns round by round in one process, so that
clock and thermal drift hit all alike.  One call = the whole model method (input scaling, factorisation, forward, the sample kernel),
timed with HIP events after warm-up; peak memory is torch's high-water mark of allocated bytes over the call, above what was allocated
before it.  Prints the median and spread of each point, the largest difference between the two ways, then one JSON line.

    python tools/predict_quant_time.py [--rows 100000] [--topics 10] [--samples 256] [--vocab 50] [--big-vocab 4096] [--reps 10] [--warmup 3]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.kernels import RBF  # noqa: E402
from gdrf_amd.models import SparseMultinomialGDRF  # noqa: E402

QS = (0.05, 0.5, 0.95)
TAUS = (0.125, 0.25, 0.5)      # float32 values: torch compares the stored float32 samples with the threshold rounded to float32


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


def compose_quantiles(model, xs, S, seed):
    th = torch.sort(model.sample_topic_probs(xs, S, seed=seed), dim=0).values
    out = []
    for q in QS:
        h = q * (S - 1)
        lo = math.floor(h)
        a, b = th[lo].double(), th[min(lo + 1, S - 1)].double()
        out.append(a + (h - lo) * (b - a))
    return torch.stack(out)


def compose_exceedance(model, xs, S, seed):
    th = model.sample_topic_probs(xs, S, seed=seed)
    return torch.stack([(th > tau).sum(0).double() / S for tau in TAUS])


def compose_dominant(model, xs, S, seed):
    th = model.sample_topic_probs(xs, S, seed=seed)
    return torch.nn.functional.one_hot(th.argmax(-1), th.shape[-1]).sum(0).double() / S


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=50)
    ap.add_argument("--big-vocab", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, K, S, seed = a.rows, a.topics, a.samples, 1234
    xs = torch.rand(N, 2, generator=torch.Generator().manual_seed(1)).cuda()
    model, big = make_model(K, a.vocab), make_model(K, a.big_vocab)
    words16 = torch.randperm(a.big_vocab, generator=torch.Generator().manual_seed(2))[:16]
    calls = {
        "topic_probs_mc": lambda: model.topic_probs_mc(xs, S, seed=seed)[0],
        "quantiles": lambda: model.topic_probs_quantiles(xs, QS, S, seed=seed),
        "quantiles_composed": lambda: compose_quantiles(model, xs, S, seed),
        "exceedance": lambda: model.exceedance(xs, TAUS, num_samples=S, seed=seed),
        "exceedance_composed": lambda: compose_exceedance(model, xs, S, seed),
        "dominant": lambda: model.dominant_topic_probs(xs, S, seed=seed),
        "dominant_composed": lambda: compose_dominant(model, xs, S, seed),
        f"word_quantiles_V{a.vocab}": lambda: model.word_probs_quantiles(xs, QS, None, S, seed=seed),
        f"word_exceedance_V{a.vocab}": lambda: model.exceedance(xs, TAUS, "word", None, S, seed=seed),
        f"word_quantiles_V{a.big_vocab}_16": lambda: big.word_probs_quantiles(xs, QS, words16, S, seed=seed),
    }
    diffs = {k: float((calls[k]() - calls[k + "_composed"]()).abs().max()) for k in ("quantiles", "exceedance", "dominant")}
    print("largest difference between the kernel and the composition", {k: f"{v:.2e}" for k, v in diffs.items()}, flush=True)
    plans = {}
    for name in ("quantiles", f"word_quantiles_V{a.vocab}", f"word_quantiles_V{a.big_vocab}_16"):
        calls[name]()
        plans[name] = (big if name.endswith("_16") else model)._engine.last_quant_plan()
    print("plan (rows, components per workgroup pass, LDS bytes)", plans, flush=True)
    times, peak = {k: [] for k in calls}, {}
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
            assert bool(torch.isfinite(out).all()), name
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
            del out
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), peak_mb=peak[name] / 2 ** 20)
        print(f"N={N} K={K} S={S} {name:26s}: median {res[name]['median_ms']:9.3f} ms  (min {res[name]['min_ms']:.3f}, max {res[name]['max_ms']:.3f}) "
              f"over {len(t)} calls, peak {res[name]['peak_mb']:.1f} MB", flush=True)
    print(json.dumps(dict(rows=N, M=256, K=K, S=S, V=a.vocab, reps=a.reps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          **{f"diff_{k}": v for k, v in diffs.items()})))


if __name__ == "__main__":
    main()
