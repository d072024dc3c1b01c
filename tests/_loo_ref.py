"""The float64 torch restatement of PSIS leave-one-out as csrc/predict_loo.h defines it, vectorised over the rows, the tail length, and
the planning rule of csrc/forms.h::loo_plan restated in Python.  For a row with the log likelihoods a_s, s = 0 .. S-1:

    1  x_s = min(a) - a_s, ordered ascending; a_(r) = min(a) - x_(r)
    2  M = ceil(min(S / 5, 3 sqrt(S))), u = x_(S-M-1), y_i = exp(x_(S-M+i)) - exp(u)
    3  q = y_(floor(M/4 + 0.5) - 1); q not > 0: pareto_k = NaN and the tail stays; a non-finite k is returned and the tail stays
    4  m = 30 + floor(sqrt(M)); b_j = (1 - sqrt(m / (j - 0.5))) / (3 q) + 1 / y_(M-1); k_j = mean_i log1p(-b_j y_i);
       L_j = M (log(-b_j / k_j) - k_j - 1); w_j = 1 / sum_t exp(L_t - L_j), normalised; b = sum_j w_j b_j; k' = mean_i log1p(-b y_i);
       sigma = -k' / b; pareto_k = (M k' + 5) / (M + 10)
    5  tail value i -> log(sigma expm1(-k log1p(-p_i)) / k + exp(u)), p_i = (i + 0.5) / M  (k == 0: -sigma log1p(-p_i))
    6  x = min(x, 0); lw = x - logsumexp(x)
    7  elpd_loo = logsumexp(a_(r) + lw_(r)); ess = 1 / sum exp(2 lw)

(test infrastructure)."""
import math

import torch

NAMES = ("elpd_loo", "pareto_k", "ess", "lpd", "total", "log_coef")
MAX_SAMPLES, MIN_SAMPLES = 1024, 25
# the caps of the PSIS arithmetic against this restatement on the same float64 inputs: pareto_k absolute, elpd_loo over the row's largest
# |a|, ess relative.  Reordered double sums over at most 96 terms differ near 1e-13 and the fit amplifies an absolute change in a into k
# about tenfold: the caps are far above either and far below any mistake in the arithmetic.
K_CAP, ELPD_CAP, ESS_CAP = 1e-8, 1e-10, 1e-8


def tail_len(S: int) -> int:
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S))))


def fit_grid(M: int) -> int:
    return 30 + int(math.floor(math.sqrt(M)))


def psis(a: torch.Tensor) -> torch.Tensor:
    """(3, n) float64 - elpd_loo, pareto_k, ess - of the columns of a (S, n), on a's device"""
    a = a.double()
    S, n = a.shape
    M = tail_len(S)
    amin = a.min(0).values
    x = (amin[None] - a).sort(0).values
    a_ord = amin[None] - x
    t0 = S - M
    eu = torch.exp(x[t0 - 1])
    y = torch.exp(x[t0:]) - eu[None]                                         # (M, n), ascending
    q = y[int(math.floor(M / 4.0 + 0.5)) - 1]
    fit = q > 0
    m = fit_grid(M)
    one = torch.ones_like(q)
    qs, ymax = torch.where(fit, q, one), torch.where(fit, y[M - 1], one)     # rows without a fit: any finite stand-in, masked below
    j = torch.arange(1, m + 1, dtype=torch.float64, device=a.device)
    bj = (1.0 - torch.sqrt(m / (j - 0.5)))[:, None] / (3.0 * qs)[None] + (1.0 / ymax)[None]      # (m, n)
    kj = torch.log1p(-bj[:, None, :] * y[None]).sum(1) / M
    L = M * (torch.log(-bj / kj) - kj - 1.0)
    w = 1.0 / torch.exp(L[None, :, :] - L[:, None, :]).sum(1)                 # w[j] = 1 / sum_t exp(L[t] - L[j])
    w = w / w.sum(0, keepdim=True)
    b = (w * bj).sum(0)
    kp = torch.log1p(-b[None] * y).sum(0) / M
    sigma = -kp / b
    k = torch.where(fit, (M * kp + 5.0) / (M + 10.0), torch.full_like(q, float("nan")))
    smooth = fit & torch.isfinite(k)
    lp = torch.log1p(-(torch.arange(M, dtype=torch.float64, device=a.device) + 0.5) / M)[:, None]
    ks = torch.where(smooth & (k != 0), k, one)
    qt = torch.where((k == 0)[None], -sigma[None] * lp, sigma[None] * torch.expm1(-ks[None] * lp) / ks[None])
    xs = x.clone()
    xs[t0:] = torch.where(smooth[None], torch.log(qt + eu[None]), x[t0:])
    xs = xs.clamp_max(0.0)
    lw = xs - torch.logsumexp(xs, 0)[None]
    return torch.stack([torch.logsumexp(a_ord + lw, 0), k, 1.0 / torch.exp(2.0 * lw).sum(0)])


def errors(got: torch.Tensor, ref: torch.Tensor, a: torch.Tensor) -> dict:
    """The figures the PSIS arithmetic is held to, rows 0 .. 2 of ``got`` against ``ref`` = psis(a): ``pareto_k`` the largest absolute
    error where the restatement is not NaN, ``elpd_loo`` the largest error over the row's largest |a| (1 where that is smaller),
    ``ess`` the largest relative error, and ``nan`` the rows where only one of the two has a NaN pareto_k."""
    got, ref, a = got.double().cpu(), ref.double().cpu(), a.double().cpu()
    nan_g, nan_r = torch.isnan(got[1]), torch.isnan(ref[1])
    ok = ~nan_r & ~nan_g
    scale = a.abs().max(0).values.clamp_min(1.0)
    return dict(pareto_k=float((got[1] - ref[1])[ok].abs().max()) if bool(ok.any()) else 0.0,
                elpd_loo=float(((got[0] - ref[0]).abs() / scale).max()), ess=float(((got[2] - ref[2]).abs() / ref[2]).max()),
                nan=int((nan_g != nan_r).sum()))


def within_caps(figs: dict) -> bool:
    return figs["nan"] == 0 and figs["pareto_k"] <= K_CAP and figs["elpd_loo"] <= ELPD_CAP and figs["ess"] <= ESS_CAP


def gpd_tail_rows(S: int, ks) -> torch.Tensor:
    """(S, len(ks)) log likelihoods whose importance ratios r_s = exp(-a_s) lie on exact generalised-Pareto quantiles (sigma = 1) at
    U_i = (i + 0.5) / S: r = ((1 - U)^-k - 1) / k + 1 (k = 0: 1 - log(1 - U)), so the whole sample, hence its tail, is GPD(k)"""
    U = (torch.arange(S, dtype=torch.float64) + 0.5) / S
    cols = []
    for k in ks:
        r = 1.0 - torch.log1p(-U) if k == 0 else torch.expm1(-k * torch.log1p(-U)) / k + 1.0
        cols.append(-torch.log(r))
    return torch.stack(cols, 1)


# ---- csrc/forms.h::loo_plan
LDS_MAX, LDS_ROWS, WG_CU, STAGE_WG_CU, V_CHUNK = 160 * 1024, 150 * 1024, 2, 3, 128


def lane_group(K: int) -> int:
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def loo_plan(K: int, V: int, S: int, esz: int, LG: int, csr: bool):
    """(RP, P, M, stride, lds): the rows of a workgroup pass that put the most rows in flight on a compute unit - which holds WG_CU workgroups of
    the fused kernel, STAGE_WG_CU of the stage kernel (K = 0), where their LDS fits -, the larger RP among equals"""
    RPB, Kp, W = 256 // LG, (K + LG - 1) // LG * LG, min(V, V_CHUNK)
    P = 1
    while P < S:
        P <<= 1
    M = tail_len(S)
    stride = P + M + 3 * fit_grid(M)
    fixed = 0 if csr else K * W * esz
    row = stride * 8 + Kp * esz + (0 if csr else W * 4)
    best, best_rows = (1, fixed + row), 0
    for rp in range(1, RPB + 1):
        lds = fixed + rp * row
        if lds > LDS_ROWS:
            break
        rows = rp * min(WG_CU if K else STAGE_WG_CU, LDS_MAX // lds)
        if rows >= best_rows:
            best, best_rows = (rp, lds), rows
    return best[0], P, M, stride, best[1]


PSIS_LG = 16      # the stage kernel's group


def stage_plan(S: int):
    return loo_plan(0, 0, S, 0, PSIS_LG, True)
