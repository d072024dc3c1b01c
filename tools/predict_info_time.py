"""Time of the entropy and information-gain maps (SparseMultinomialGDRF.information, csrc/predict_info.h) beside the torch composition a
user had before it.

float32 arrays with the f64 solve, N = 1e5 rows, M = 256 inducing points (16 x 16 grid), K = 10 topics, S = 64 Philox samples, D = 2, at
V = 50 and V = 4096 words.  The composition - on the smaller vocabulary only, where its S x piece x V intermediate fits - is
sample_topic_probs (S x N x K stored), then `@ word_topic_matrix` and the entropies with torch in row pieces.  Two yardsticks on the first
vocabulary say where information()'s time goes: forward (the mode-4 forward every predictive call starts with) and topic_probs_mc (the
forward plus one generation of the S draws and their softmax, which information() repeats for every chunk of GDRF_INFO_V_CHUNK words).
The calls take turns round by round in one process, so that clock and thermal drift hit all alike.  One call = the whole model method
(input scaling, factorisation, forward, the sample kernel), timed with HIP events after warm-up.  Prints the median and spread of each
point and the largest difference between the two ways, then one JSON line.

    python tools/predict_info_time.py [--rows 100000] [--topics 10] [--samples 64] [--vocab 50 4096] [--compose-up-to 50] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrf_amd.engine import INFO_NAMES  # noqa: E402
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


def entropy(q):
    return -torch.where(q > 0, q * q.clamp_min(1e-38).log(), torch.zeros_like(q)).double().sum(-1)


def compose(model, xs, S, seed):
    """the six maps from stored samples with torch: theta (S, N, K) once, p (S, piece, V) piece by piece"""
    theta = model.sample_topic_probs(xs, S, seed=seed)
    phi = model.word_topic_matrix.to(theta)
    tb = theta.mean(0)
    te, tx = entropy(tb), entropy(theta).mean(0)
    we, wx = [], []
    for a in range(0, xs.shape[0], PIECE):
        we.append(entropy(tb[a:a + PIECE] @ phi))
        wx.append(entropy(theta[:, a:a + PIECE] @ phi).mean(0))
    we, wx = torch.cat(we), torch.cat(wx)
    return dict(zip(INFO_NAMES, (te, tx, te - tx, we, wx, we - wx)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--topics", type=int, default=10)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--vocab", type=int, nargs="*", default=[50, 4096])
    ap.add_argument("--compose-up-to", type=int, default=50, help="the largest V at which the torch composition is run as well")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, K, S = a.rows, a.topics, a.samples
    xs = torch.rand(N, 2, generator=torch.Generator().manual_seed(1)).cuda()
    calls, diffs = {}, {}
    for V in a.vocab:
        model = make_model(K, V)
        if not calls:
            calls[f"forward_V{V}"] = lambda model=model: dict(zip(("loc", "var"), model.forward(xs)))
            calls[f"topic_probs_mc_V{V}"] = lambda model=model: dict(zip(("mean", "var"), model.topic_probs_mc(xs, S, seed=1234)))
        calls[f"information_V{V}"] = lambda model=model: model.information(xs, S, seed=1234)
        if V <= a.compose_up_to:
            calls[f"composition_V{V}"] = lambda model=model: compose(model, xs, S, 1234)
            got, want = calls[f"information_V{V}"](), calls[f"composition_V{V}"]()
            diffs[V] = {k: float((got[k] - want[k]).abs().max()) for k in INFO_NAMES}
            print(f"V={V}: largest difference between information() and the composition", {k: f"{v:.2e}" for k, v in diffs[V].items()}, flush=True)
    times = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in out.values()), name
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {}
    for name, t in times.items():
        res[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f"N={N} K={K} S={S} {name:20s}: median {res[name]['median_ms']:.3f} ms  (min {res[name]['min_ms']:.3f}, "
              f"max {res[name]['max_ms']:.3f}) over {len(t)} calls", flush=True)
    print(json.dumps(dict(rows=N, M=256, K=K, S=S, reps=a.reps, **{f"{k}_{q}": v for k, r in res.items() for q, v in r.items()},
                          **{f"diff_V{V}_{k}": v for V, d in diffs.items() for k, v in d.items()})))


if __name__ == "__main__":
    main()
