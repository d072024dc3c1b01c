"""GPU tests of the Monte-Carlo predictive path (gdrf_predict_mc, csrc/predict_mc.h) against a float64 torch restatement of its
definition, written in tests/_mc_util.py from oracle.gdrf_oracle.conditional and the model's parameters:

    mu[s,k,n] = f_loc[k,n] + mean[k,n] + f_var[k,n] eps[s,k,n];  theta[s,n,:] = softmax_k(mu[s,:,n]);  p[s,n,:] = theta[s,n,:] Phi
    l_n = logsumexp_s(sum_v w[n,v] log p[s,n,v]) - log S

Tolerances are those of the predictive path (tests/test_gpu_parity.py::test_predictive_path): 1e-9 in fp64 contexts, 5e-4 in float32
ones, relerr = max-abs over max-abs.  float32 contexts are compared with the float64 restatement at the same float32-valued parameters
and the same jitter level.  The model is the grid model M = 20 (n_points = (5, 4)), V = 9, with perturbed u_loc / phi_unc and a
contracted, perturbed u_scale_tril, so that f_var is neither 0 nor constant.
"""
import copy
import math

import numpy as np
import pytest
import torch

from tests._mc_util import MEAN_KN, _model, build, engine, loc_var, restate
from tests._util import dev, relerr

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-9, torch.float32: 5e-4}
DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
NS, KS, SS = (1, 63, 257), (1, 2, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128), (1, 2, 7, 64)      # KS: the last K of every lane-group form and the first of the next


def check_modes(eng, m, xs, ws, eps, tol, mean=None, report=None):
    """modes 0-3 with injected eps against the restatement; rows of theta sum to one"""
    S, K, n = eps.shape
    mu_r, th_r, sc_r = restate(m, xs, eps, ws)
    xd, wd, ed = dev(xs, eng), dev(ws, eng, torch.int32), dev(eps, eng)
    mu = eng.predict_mc(xd, 3, S, eps=ed, mean=mean).cpu()
    th = eng.predict_mc(xd, 0, S, eps=ed, mean=mean).cpu()
    mv = eng.predict_mc(xd, 1, S, eps=ed, mean=mean).cpu()
    sc = eng.predict_mc(xd, 2, S, ws=wd, eps=ed, mean=mean).cpu().numpy()
    assert mu.shape == (S, K, n) and th.shape == (S, n, K) and mv.shape == (2, n, K)
    figs = dict(mu=relerr(mu.numpy(), mu_r.numpy()), theta=relerr(th.numpy(), th_r.numpy()),
                mean=relerr(mv[0].numpy(), th_r.mean(0).numpy()),
                var=relerr(mv[1].numpy(), th_r.var(0, unbiased=False).numpy()),
                score=abs(sc[0] - sc_r[0]) / abs(sc_r[0]), wsum=abs(sc[1] - sc_r[1]),
                rowsum=float((th.double().sum(-1) - 1).abs().max()) / float(torch.finfo(eng.dtype).eps))
    print(f"K={K} n={n} S={S} {eng.dtype}", {k: f"{v:.2e}" for k, v in figs.items()})
    if report is not None:
        report.append(figs)
    assert figs["mu"] < tol and figs["theta"] < tol and figs["mean"] < tol and figs["var"] < tol and figs["score"] < tol, figs
    assert figs["wsum"] == 0.0, figs
    assert figs["rowsum"] <= 4 * K, figs                                    # within 4 K ulps of the array dtype


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", KS)
def test_injected_eps_parity_every_mode_and_shape(K, dtype):
    m = build(K, max(NS), dtype)
    eng = engine(m, dtype)
    g = torch.Generator().manual_seed(7)
    for n in NS:
        for S in SS:
            eps = torch.randn(S, K, n, generator=g, dtype=torch.float64).to(dtype)
            check_modes(eng, m, m.xs[:n].contiguous(), m.ws[:n].contiguous(), eps, TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["mean_function", "unwhitened", "matern52"])
def test_injected_eps_parity_mean_unwhitened_and_matern(variant, dtype):
    mean_fn = MEAN_KN if variant == "mean_function" else None          # (K, n): another shift for every topic
    m = build(5, 63, dtype, kind="matern52" if variant == "matern52" else "rbf", whiten=variant != "unwhitened", mean_function=mean_fn)
    eng = engine(m, dtype)
    eps = torch.randn(7, 5, 63, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    mean = None if mean_fn is None else dev(mean_fn(m.xs), eng)
    check_modes(eng, m, m.xs, m.ws, eps, TOL[dtype], mean=mean)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_sample_with_zero_eps_is_the_plug_in(dtype):
    m = build(5, 257, dtype)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    zero = torch.zeros(1, 5, 257, dtype=dtype, device=eng.device)
    assert relerr(eng.predict_mc(xs, 0, 1, eps=zero)[0].cpu().numpy(), eng.predict(xs, 1).cpu().numpy()) < TOL[dtype]
    a, b = eng.predict_mc(xs, 2, 1, ws=ws, eps=zero).cpu().numpy(), eng.predict(xs, 3, ws).cpu().numpy()
    assert abs(a[0] - b[0]) / abs(b[0]) < TOL[dtype] and a[1] == b[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,n,S,off", [(5, 63, 7, 1000), (128, 257, 2, 2 ** 33 + 5), (2, 1, 64, 0),
                                        (33, 4101, 2, 7)])          # 4 rows per workgroup, 1024 workgroups: the first ones take a second trip
def test_philox_draws_equal_their_own_injection_bitwise(K, n, S, off, dtype):
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs = dev(m.xs, eng)
    seed = 0x1234ABCD5678
    E = torch.stack([eng.fill_eps(seed, s, off, n) for s in range(S)]).contiguous()
    for mode in (0, 1, 3):
        a = eng.predict_mc(xs, mode, S, seed=seed, row_offset=off)
        b = eng.predict_mc(xs, mode, S, eps=E)
        assert torch.equal(a, b), mode


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_results_do_not_depend_on_how_the_rows_are_batched(dtype):
    K, n, S, a = 5, 257, 7, 100
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    for mode in (0, 1):
        one = eng.predict_mc(xs, mode, S, seed=11)
        two = torch.cat([eng.predict_mc(xs[:a], mode, S, seed=11), eng.predict_mc(xs[a:], mode, S, seed=11, row_offset=a)], dim=1)
        assert torch.equal(one, two), mode
    one = eng.predict_mc(xs, 2, S, ws=ws, seed=11).cpu().numpy()
    two = (eng.predict_mc(xs[:a], 2, S, ws=ws[:a], seed=11) + eng.predict_mc(xs[a:], 2, S, ws=ws[a:], seed=11, row_offset=a)).cpu().numpy()
    print("score", one, two)
    assert one[1] == two[1]
    assert abs(one[0] - two[0]) / abs(one[0]) < (1e-12 if dtype == torch.float64 else TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_surface_cuts_rows_into_pieces_without_changing_the_result(dtype, monkeypatch):
    import gdrf_amd.models.sparse_gdrf as sg
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 80)         # a call grows an engine to at most this many rows: `small` stays at 80
    K, n, S = 5, 257, 7
    mean_fn = MEAN_KN
    m = build(K, n, dtype, mean_function=mean_fn)
    small, big = _model(m, dtype, 80, mean_function=mean_fn), _model(m, dtype, n, mean_function=mean_fn)
    assert small._engine.n_cap < n / 3 and big._engine.n_cap == n
    xs, ws = m.xs.to(dtype), m.ws
    th = big.sample_topic_probs(xs, S, seed=3)
    assert th.shape == (S, n, K) and torch.equal(th, small.sample_topic_probs(xs, S, seed=3))
    mean, var = big.topic_probs_mc(xs, S, seed=3)
    mean_s, var_s = small.topic_probs_mc(xs, S, seed=3)
    assert mean.shape == (n, K) and torch.equal(mean, mean_s) and torch.equal(var, var_s)
    # seed=None is the model's rng_seed; the moments are those of the samples; the word distribution is mean @ Phi
    assert torch.equal(big.sample_topic_probs(xs, 2), big.sample_topic_probs(xs, 2, seed=big.rng_seed))
    assert relerr(mean.cpu().numpy(), th.double().mean(0).cpu().numpy()) < TOL[dtype]
    assert relerr(var.cpu().numpy(), th.double().var(0, unbiased=False).cpu().numpy()) < TOL[dtype]
    assert torch.equal(big.word_probs_mc(xs, S, seed=3), mean @ big.word_topic_matrix)
    pa, pb = float(big.predictive_perplexity(xs, ws, S, seed=3)), float(small.predictive_perplexity(xs, ws, S, seed=3))
    assert big.predictive_perplexity(xs, ws, S, seed=3).dim() == 0
    assert abs(pa - pb) / pa < (1e-12 if dtype == torch.float64 else TOL[dtype])
    # against the restatement, with the mean_function, through injected draws cut into the same pieces
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype)
    m.force_jitter_level = big._engine.last_jitter_level
    _, th_r, sc_r = restate(m, m.xs, eps, m.ws)
    assert relerr(small.sample_topic_probs(xs, S, eps=eps).cpu().numpy(), th_r.numpy()) < TOL[dtype]
    # a restored snapshot offers the same methods; a custom link runs on the mu samples with torch
    snap = copy.deepcopy(big)
    assert snap.restore(mean_function=mean_fn)._engine.n_cap == 1        # grown by the call, to MC_PIECE_ROWS: pieces again
    assert relerr(snap.restore(mean_function=mean_fn).topic_probs_mc(xs, S, seed=3)[0].cpu().numpy(), mean.cpu().numpy()) < TOL[dtype]
    for name in ("sample_topic_probs", "topic_probs_mc", "word_probs_mc", "predictive_perplexity"):
        assert callable(getattr(snap, name))
    linked = _model(m, dtype, 80, link_function=lambda mu: torch.softmax(mu, -2), mean_function=mean_fn)
    assert relerr(linked.sample_topic_probs(xs, S, eps=eps).cpu().numpy(), th_r.numpy()) < TOL[dtype]
    lm, lv = linked.topic_probs_mc(xs, S, seed=3)
    assert relerr(lm.cpu().numpy(), mean.cpu().numpy()) < TOL[dtype] and relerr(lv.cpu().numpy(), var.cpu().numpy()) < TOL[dtype]
    with pytest.raises(NotImplementedError):
        linked.predictive_perplexity(xs, ws, S)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_free_running_generator_known_answer(dtype):
    """K = 2: theta_0 = sigmoid(d), d ~ N(loc_0 - loc_1, var_0^2 + var_1^2) (f_var is the scale).  Its mean by Gauss-Hermite quadrature
    (128 nodes, float64); mode 1's mean must lie within 6 standard errors 6 sqrt(var_reported / S) of it.  16 entries, fixed seed: a
    correct generator fails by chance with probability < 16 * 2e-9.  The scale of d is 5 - 11 here (prior variance 25), where the 128- and
    64-node rules differ by 2e-3: the quadrature's own error is a twentieth of the bound (6 standard errors are about 0.04)."""
    K, n, S = 2, 8, 4096
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    loc, var = loc_var(m, m.xs)
    d_loc, d_sd = (loc[0] - loc[1]).numpy(), (var[0] ** 2 + var[1] ** 2).sqrt().numpy()
    x, w = np.polynomial.hermite.hermgauss(128)
    e0 = (w[None] / (1.0 + np.exp(-(d_loc[:, None] + math.sqrt(2.0) * d_sd[:, None] * x[None])))).sum(1) / math.sqrt(math.pi)
    want = np.stack([e0, 1.0 - e0], axis=1)                                 # (n, K)
    mv = eng.predict_mc(dev(m.xs, eng), 1, S, seed=20240229).cpu().double().numpy()
    se = np.sqrt(mv[1] / S)
    z = np.abs(mv[0] - want) / se
    print("sd of d", d_sd, "z", z.max(), "se", se.max())
    assert (d_sd > 0.05).all() and (se > 0).all()
    assert (z <= 6.0).all(), z


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_step_is_bitwise_the_same_after_predict_mc(dtype):
    K, n = 5, 63
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    eps = dev(torch.randn(K, n, generator=torch.Generator().manual_seed(4), dtype=torch.float64), eng)

    def step():
        eng.loss_and_grads(xs, ws, eps)
        return eng.out_d.clone(), eng.grads.clone()

    step()
    out1, g1 = step()
    other = xs[:40].contiguous()
    for mode in (0, 1, 2, 3):
        eng.predict_mc(other, mode, 3, ws=ws[:40].contiguous() if mode == 2 else None, seed=1, mean=dev(torch.ones(40), eng))
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)


def test_limits():
    from gdrf_amd._lib import GdrfHipError
    m = build(5, 63, torch.float64)
    eng = engine(m, torch.float64, n_cap=32)
    with pytest.raises(ValueError, match="n_cap"):
        eng.predict_mc(dev(m.xs, eng), 0, 2, seed=1)
    big = build(128, 8, torch.float32, V=400)                               # Phi alone is 200 KB
    eng = engine(big, torch.float32)
    xs, ws = dev(big.xs, eng), dev(big.ws, eng, torch.int32)
    with pytest.raises(GdrfHipError, match="too large"):
        eng.predict_mc(xs, 2, 2, ws=ws, seed=1)
    assert eng.predict_mc(xs, 1, 2, seed=1).shape == (2, 8, 128)            # the modes without Phi have no such limit
