"""Float64 restatement of the credible-interval, exceedance and dominant-topic maps (gdrf_predict_quant, csrc/predict_quant.h) from an
(S, n, C) sample array, CPU only, and of the quantile mode's planning rule, written from its description:

  quantiles   type 7 ("linear"): h = q (S - 1), lo = floor(h), hi = min(lo + 1, S - 1), frac = h - lo, x_(lo) + frac (x_(hi) - x_(lo))
  exceedance  #{s : x_s > tau} / S, strict
  dominant    #{s : argmax_k theta_s = k} / S, equal values to the lower index
"""
import math

import numpy as np
import torch

QUANT_LDS = 64 * 1024
MAX_SAMPLES, MAX_LEVELS = 1024, 16
# (K, S, element size) -> (RP, CP, lds) of the GPU cases that name their plan (topics: C = K), the two ends of the rule at 1024 samples:
# a row of 8 topics in double, where a component's samples take 8 KB and 7 of the 32 groups get a row, and rows of 128 topics, where
# the four groups' rows share the room with several components per pass and the last pass is ragged.  tests/test_quant_plan_host.py
# holds the table program to them, tests/test_gpu_predict_quant.py the launch.
GPU_PLANS = {(8, 1024, 8): (7, 1, 59896), (128, 1024, 4): (3, 5, 64316), (128, 1024, 8): (1, 7, 62008)}


def lo_frac(q: float, S: int):
    h = float(q) * (S - 1)
    lo = math.floor(h)
    return int(lo), h - lo


def quantiles_ref(x: torch.Tensor, qs) -> torch.Tensor:
    """(Q, n, C) float64 from samples x of shape (S, n, C)"""
    xs = torch.sort(x.double(), dim=0).values
    S = xs.shape[0]
    out = []
    for q in qs:
        lo, frac = lo_frac(q, S)
        hi = min(lo + 1, S - 1)
        out.append(xs[lo] + frac * (xs[hi] - xs[lo]))
    return torch.stack(out)


def quantile_ends(x: torch.Tensor, qs):
    """max(|x_(lo)|, |x_(hi)|) per level, (Q, n, C): what the interpolation's roundings are bounded by"""
    xs = torch.sort(x.double(), dim=0).values
    S = xs.shape[0]
    out = []
    for q in qs:
        lo, _ = lo_frac(q, S)
        out.append(torch.maximum(xs[lo].abs(), xs[min(lo + 1, S - 1)].abs()))
    return torch.stack(out)


def exceed_counts_ref(x: torch.Tensor, taus) -> torch.Tensor:
    """(Tn, n, C) int64 counts of x_s > tau"""
    xd = x.double()
    return torch.stack([(xd > float(t)).sum(0) for t in taus])


def exceed_ref(x: torch.Tensor, taus) -> torch.Tensor:
    return exceed_counts_ref(x, taus).double() / x.shape[0]


def dominant_counts_ref(th: torch.Tensor) -> torch.Tensor:
    """(n, K) int64 counts of argmax_k theta_s = k, the first of equal values (numpy's argmax)"""
    S, n, K = th.shape
    idx = torch.from_numpy(np.argmax(th.double().numpy(), axis=2))
    return torch.nn.functional.one_hot(idx, K).sum(0)


def dominant_ref(th: torch.Tensor) -> torch.Tensor:
    return dominant_counts_ref(th).double() / th.shape[0]


def lane_group(K: int) -> int:
    """lanes that own a row in the predictive lane-group kernels"""
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def quant_plan(K: int, C: int, S: int, esz: int, LG: int):
    """(RP, CP, lds) of the quantile mode: LDS holds theta [256 / LG][Kp] and samples [RP][CP (P + 1) + LG] elements of esz bytes within
    64 KB; among RP = 1 .. 256 / LG with CP the most components (at most C) that fit beside RP rows, the pair with the least
    ceil(C / CP) / RP, the larger RP among equals."""
    RPB = 256 // LG
    Kp = -(-K // LG) * LG
    P = 1
    while P < S:
        P *= 2
    theta = RPB * Kp * esz

    def lds(rp, cp):
        return theta + rp * (cp * (P + 1) + LG) * esz

    best = None
    for rp in range(1, RPB + 1):
        cp = 0
        while cp < C and lds(rp, cp + 1) <= QUANT_LDS:
            cp += 1
        if cp == 0:
            break
        passes = -(-C // cp)
        if best is None or passes * best[0] <= best[2] * rp:
            best = (rp, cp, passes)
    return best[0], best[1], lds(best[0], best[1])
