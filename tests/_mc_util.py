"""What the GPU tests of the Monte-Carlo predictive calls share: the float64 oracle model they run on - the grid model M = 20
(n_points = (5, 4)), V = 9, with perturbed u_loc / phi_unc and a contracted, perturbed u_scale_tril, so that f_var is neither 0 nor
constant -, the float64 torch restatement of the draws from oracle.gdrf_oracle.conditional and the model's parameters

    mu[s,k,n] = f_loc[k,n] + mean[k,n] + f_var[k,n] eps[s,k,n];  theta[s,n,:] = softmax_k(mu[s,:,n]);  p[s,n,:] = theta[s,n,:] Phi
    l_n = logsumexp_s(sum_v w[n,v] log p[s,n,v]) - log S

and an engine or a device model with the oracle's parameters (test infrastructure; may import oracle/)."""
import math

import torch

from oracle.gdrf_oracle import RefShapedGDRF, conditional
from tests._util import engine_from_oracle

V, NPTS = 9, (5, 4)


def build(K, n, dtype, kind="rbf", whiten=True, mean_function=None, seed=0, V=V):
    """The float64 oracle model on n random rows (its parameters rounded to float32 values for a float32 context)."""
    g = torch.Generator().manual_seed(1000 * K + n + seed)
    xs = torch.rand(n, 2, generator=g, dtype=torch.float64)
    ws = torch.randint(0, 7, (n, V), generator=g, dtype=torch.int32)
    ws[torch.rand(n, V, generator=g) < 0.4] = 0
    m = RefShapedGDRF(xs, ws, kind=kind, K=K, n_points=NPTS, lengthscale=0.3, variance=25.0, dtype=torch.float64,
                      jitter=1e-6 if dtype == torch.float64 else 1e-4, whiten=whiten, mean_function=mean_function)
    with torch.no_grad():
        p = m.params
        p["u_loc"].add_(0.5 * torch.randn(p["u_loc"].shape, generator=g, dtype=torch.float64))
        u = 0.1 * torch.randn(p["u_scale_tril_unc"].shape, generator=g, dtype=torch.float64).tril(-1)
        p["u_scale_tril_unc"].copy_(u + torch.diag_embed(torch.full(p["u_loc"].shape, math.log(0.3), dtype=torch.float64)))
        p["phi_unc"].add_(0.5 * torch.randn(p["phi_unc"].shape, generator=g, dtype=torch.float64))
        if dtype == torch.float32:
            for v in p.values():
                v.copy_(v.float().double())
    return m


def loc_var(m, xs):
    """(f_loc + mean, f_var) of the oracle at rows xs, float64, (K, n) each"""
    c = m.constrained()
    with torch.no_grad():
        loc, var = conditional(m.kind, xs, m.inducing(), c["lengthscale"], c["variance"], c["u_loc"], c["u_scale_tril"], m._luu(c),
                               c["scale_mixture"], m.whiten)
        if m.mean_function is not None:
            loc = loc + m.mean_function(xs)
    return loc, var


def restate(m, xs, eps, ws=None):
    """mu (S, K, n), theta (S, n, K) and, with counts, (sum_n l_n, sum w) of the definition, in float64"""
    loc, var = loc_var(m, xs)
    mu = loc[None] + var[None] * eps.double()
    theta = torch.softmax(mu, dim=1).transpose(1, 2)
    score = None
    if ws is not None:
        with torch.no_grad():
            p = theta @ m.constrained()["phi"]
        lp = (ws.double()[None] * p.log()).sum(-1)                          # (S, n)
        score = (float((torch.logsumexp(lp, 0) - math.log(eps.shape[0])).sum()), float(ws.double().sum()))
    return mu, theta, score


def MEAN_KN(x):
    """a mean_function for K = 5 that differs between the topics (a shift common to all of them would cancel in the softmax)"""
    k = torch.arange(5, dtype=x.dtype, device=x.device)[:, None]
    return (0.7 - 0.5 * k) * x[None, :, 0] + 0.4 * (k - 2.0) * x[None, :, 1] ** 2


def engine(m, dtype, n_cap=None):
    eng = engine_from_oracle(m, dtype=dtype, n_cap=n_cap)
    m.force_jitter_level = eng.factorize()
    return eng


def _model(m, dtype, n_cap, link_function=None, mean_function=None):
    """A SparseMultinomialGDRF with the oracle's parameters and inducing inputs (the oracle lays its grid out in float32, the model in
    float64: the same points to 1e-8 only) whose engine holds n_cap rows"""
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    model = SparseMultinomialGDRF(xs=m.xs[:n_cap], ws=m.ws[:n_cap], world=[(0.0, 1.0)] * 2, num_observation_categories=m.V,
                                  kernel=RBF(input_dim=2, lengthscale=torch.tensor(0.3), variance=torch.tensor(25.0)),
                                  num_topic_categories=m.K, dirichlet_param=0.01, n_points=list(NPTS), fixed_inducing_points=True,
                                  inducing_points=m.Z, jitter=m.jitter, maxjitter=15, dtype=dtype, seed=5, device="cuda:0",
                                  link_function=link_function, mean_function=mean_function)
    for name in model._engine.PARAM_NAMES:
        model._engine.view(name).copy_(m.params[name].detach().to(dtype))
    return model
