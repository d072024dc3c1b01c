"""The float64 torch restatement of the per-row Monte-Carlo log predictive densities (gdrf_predict_score, csrc/predict_score.h), built
from oracle.gdrf_oracle.conditional and the model's parameters exactly as tests/_mc_util.py::restate builds theta:

    mu[s,k,n] = f_loc[k,n] + mean[k,n] + f_var[k,n] eps[s,k,n];  theta_s = softmax_k(mu[s]);  p_s = theta_s Phi
    a[s,n] = sum_{v: w[n,v] != 0} w[n,v] log p[s,n,v]
    lpd = logsumexp_s a - log S;  mean_log_lik = mean_s a;  var_log_lik = var_s a (unbiased, 0 for S = 1)
    total = sum_v w;  log_coef = lgamma(total + 1) - sum_v lgamma(w + 1)

(test infrastructure; may import oracle/)."""
import math

import torch

from tests._mc_util import restate

NAMES = ("lpd", "mean_log_lik", "var_log_lik", "total", "log_coef")
LPD, MLL, VLL, TOT, COEF = range(5)
TOL = {torch.float64: 1e-9, torch.float32: 5e-4}      # the predictive path's, max-abs error over max-abs value


def counts(n, V, seed, top=10000):
    """(n, V) int32 counts whose row totals run up to about ``top`` (row 0 has it; the others a uniform share of it), with about 40 % of
    the words absent from a row; the last row is empty when n > 2"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, V, generator=g, dtype=torch.float64)
    r[torch.rand(n, V, generator=g) < 0.4] = 0
    r[:, 0] += 1e-3                                                          # no row without any word
    target = torch.randint(1, top + 1, (n,), generator=g).double()
    target[0] = top
    ws = torch.floor(r / r.sum(-1, keepdim=True) * target[:, None]).to(torch.int32)
    if n > 2:
        ws[-1] = 0
    return ws


def log_liks(m, xs, ws, eps) -> torch.Tensor:
    """a (S, n) float64 of the oracle model m at rows xs with dense counts ws (n, V) under the injected draws eps (S, K, n)"""
    _, theta, _ = restate(m, xs, eps)                                       # (S, n, K)
    with torch.no_grad():
        phi = m.constrained()["phi"].double()
    w = ws.double()
    S, n = theta.shape[:2]
    a = torch.zeros(S, n, dtype=torch.float64)
    step = max(1, 2 ** 24 // (n * w.shape[1]))                              # samples at a time: at most 16M elements of (s, n, V)
    for s in range(0, S, step):
        lp = (theta[s:s + step] @ phi).log()
        a[s:s + step] = torch.where(w != 0, w * lp, torch.zeros_like(lp)).sum(-1)
    return a


def stats(a: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """(5, n) float64, rows in the order of NAMES, from the log likelihoods a (S, n) and the dense counts ws"""
    S = a.shape[0]
    w = ws.double()
    tot = w.sum(-1)
    var = a.var(0, unbiased=True) if S > 1 else torch.zeros_like(tot)
    return torch.stack([torch.logsumexp(a, 0) - math.log(S), a.mean(0), var, tot, torch.lgamma(tot + 1) - torch.lgamma(w + 1).sum(-1)])


def score_ref(m, xs, ws, eps) -> torch.Tensor:
    return stats(log_liks(m, xs, ws, eps), ws)


def errors(out: torch.Tensor, ref: torch.Tensor, one_word: float = 0.0) -> dict:
    """The figures a case is held to: ``lpd`` and ``mean_log_lik`` as max-abs error over max-abs value (an all-empty case, where the
    value is 0: the absolute error), ``var_log_lik`` as max-abs error over the case's largest var_log_lik - or, where that is smaller,
    over 2^-52 max|mean_log_lik|^2, below which a variance of sums of that size is not resolved in double (K = 1 and eps = 0, where it is
    0) -, ``total`` as the largest absolute error (it is exact) and ``log_coef`` as max-abs over max-abs.
    ``one_word`` (V = 1; 0: not so): p = sum_k theta_k = 1, every a_s is exactly 0 and the restatement returns its own rounding of it,
    about 1e-16 per token, so an error relative to that value measures nothing (tests/_info_ref.py::errors meets the same case).  The
    argument is then u, the most |p - 1| can be in the array precision: (K + 8) eps(T), K - 1 additions of terms below 1 and the few
    roundings of each theta_k (the bound tests/test_gpu_predict_quant.py gives a word's p).  a_s = w log p is at most top u in size, top
    the largest total, so the lpd and mean_log_lik errors are taken over top - the size of w x p, as before -, and the var_log_lik
    error over (top u)^2, the most a variance of such a_s can be: that figure is held to 1, not to the relative tolerance."""
    out, ref = out.double().cpu(), ref.double().cpu()
    top = float(ref[TOT].max())
    rel = lambda i: float((out[i] - ref[i]).abs().max()) / (float(ref[i].abs().max()) or 1.0)
    val = lambda i: float((out[i] - ref[i]).abs().max()) / top if one_word else rel(i)
    floor = (top * one_word) ** 2 if one_word else max(float(ref[VLL].max()), 2.0 ** -52 * float(ref[MLL].abs().max()) ** 2)
    return dict(lpd=val(LPD), mean_log_lik=val(MLL), var_log_lik=float((out[VLL] - ref[VLL]).abs().max()) / (floor or 1.0),
                total=float((out[TOT] - ref[TOT]).abs().max()), log_coef=rel(COEF))
