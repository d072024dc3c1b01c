"""Products of RBF and Periodic kernels (and lone kernels on a subset of the axes) on the GPU, against autograd through the reference-shaped
CPU oracle with pyro's formulas for the factors (pyro 1.8.0 contrib/gp/kernels/isotropic.py RBF, periodic.py Periodic):

    RBF:       variance * exp(-0.5 sum_d ((x_d - z_d) / lengthscale_d)^2)
    Periodic:  variance * exp(-2 sum_d sin^2(pi (x_d - z_d) / period_d) / lengthscale_d^2)
    Product:   kern0(X, Z) * kern1(X, Z), each factor reading its own active_dims

The oracle is RefShapedGDRF turned into a product by set_factors (oracle/gdrf_oracle.py::product_matrix): the variance it hands kernel_diag
is the product of the factors' variances."""
import copy
import os

import numpy as np
import pytest
import torch

import oracle.gdrf_oracle as go
from oracle.gdrf_oracle import product_matrix
from tests._util import (LOSS_TOL_VS_TORCH, NPTS, check_loss_and_grads, dev, engine_for, grid_inputs as inputs, load_params as load, relerr,
                         run_two_ranks, variant_oracle)

pytestmark = pytest.mark.gpu

# (name, kind, active_dims, lengthscale, variance, period) per leaf factor, pyro module paths as names
CASES = {
    "locally_periodic_1d": (1, [("kern0", "rbf", [0], 0.9, 2.0, None), ("kern1", "periodic", [0], 0.8, 1.5, 0.37)]),
    "rbf0_periodic1_2d": (2, [("kern0", "rbf", [0], 0.6, 2.0, None), ("kern1", "periodic", [1], 0.8, 1.5, 0.45)]),
    "rbf_ard01_periodic2_3d": (3, [("kern0", "rbf", [0, 1], (0.7, 1.1), 2.0, None), ("kern1", "periodic", [2], 0.8, 1.5, 0.45)]),
    "nested_three_factors_2d": (2, [("kern0.kern0", "rbf", [0], 0.7, 1.5, None), ("kern0.kern1", "periodic", [1], 0.9, 1.2, 0.4),
                                    ("kern1", "rbf", [1], 1.3, 2.0, None)]),
}


def prod_oracle(case, factors=None, D=None, **kw):
    """The oracle starts as an RBF(0.5, 1.0) one - its initial S_k is that kernel's L_uu - and takes the factors' parameters after."""
    D0, fac = CASES[case] if case else (D, factors)
    return variant_oracle(D0, lambda m: m.set_factors(fac), kind="rbf", lengthscale=0.5, variance=1.0, **kw)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("learn,whiten", [(False, True), (True, True), (False, False)])
def test_loss_and_every_gradient_fp64(case, learn, whiten):
    m, eps = prod_oracle(case, learn=learn, whiten=whiten)
    eng = engine_for(m)
    assert eng.hyper_backward == "f64" and "log_variance" not in eng.param_names
    check_loss_and_grads(eng, m, eps)


@pytest.mark.parametrize("case", list(CASES))
def test_knm_against_the_formula(case):
    m, _ = prod_oracle(case)
    fac = CASES[case][1]
    with torch.no_grad():
        ref = product_matrix(m.xs, m.Z, m.factors()).numpy()
    e64 = engine_for(m)
    assert relerr(e64.knm(dev(m.xs, e64)).cpu().numpy(), ref) < 1e-12
    e32 = engine_for(m, dtype=torch.float32)
    assert relerr(e32.knm(dev(m.xs, e32)).cpu().numpy(), ref) < 2e-6
    big = engine_for(m, n_cap=16)          # more rows than the context holds: gdrf_knm grows its scratch
    assert relerr(big.knm(dev(m.xs, big)).cpu().numpy(), ref) < 1e-12


def test_shifting_the_periodic_axis_by_one_period_leaves_knm_unchanged():
    m, _ = prod_oracle("rbf0_periodic1_2d")
    eng = engine_for(m)
    g = torch.Generator().manual_seed(2)
    xs = 0.5 * torch.rand(500, 2, generator=g, dtype=torch.float64)
    k0 = eng.knm(dev(xs, eng)).cpu().numpy()
    shift = torch.tensor([0.0, 0.45], dtype=torch.float64)
    assert relerr(eng.knm(dev(xs + shift, eng)).cpu().numpy(), k0) < 1e-13
    assert relerr(eng.knm(dev(xs + torch.tensor([0.45, 0.0], dtype=torch.float64), eng)).cpu().numpy(), k0) > 1e-3   # the RBF axis is not periodic


@pytest.mark.parametrize("case", ["locally_periodic_1d", "rbf_ard01_periodic2_3d"])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-9), (torch.float32, 5e-4)])
def test_predictive_path(case, dtype, tol):
    m, _ = prod_oracle(case, W=23, H=11, V=9, K=5)
    eng = engine_for(m, dtype=dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    m.force_jitter_level = eng.factorize()
    assert relerr(eng.predict(xs, 0).cpu().numpy(), m.log_topic_probs().detach().numpy()) < tol
    assert relerr(eng.predict(xs, 1).cpu().numpy(), m.topic_probs().detach().numpy()) < tol
    assert relerr(eng.predict(xs, 2).cpu().numpy(), m.word_probs().detach().numpy()) < tol
    s = eng.predict(xs, 3, ws).cpu().double().numpy()
    assert abs(float(np.exp(-s[0] / s[1])) - float(m.perplexity())) / float(m.perplexity()) < tol
    c = m.constrained()
    with torch.no_grad():
        loc, var = go.conditional("product", m.xs, m.inducing(), None, c["variance"], c["u_loc"], c["u_scale_tril"], m._luu(c),
                                  whiten=True, **c["kernel_kw"])
    lv = eng.predict(xs, 4).cpu()
    assert relerr(lv[0].numpy(), loc.numpy()) < tol and relerr(lv[1].numpy(), var.numpy()) < tol


def test_streamed_rows_form():
    m, eps = prod_oracle("rbf_ard01_periodic2_3d")
    eng = engine_for(m, rows_form="streamed")
    assert eng.rows_form == "streamed"
    check_loss_and_grads(eng, m, eps)


def _engine_pair(eng_b, rename):
    """Engine eng_b holds m's values under its own names (rename: its name -> tensor)."""
    for name in eng_b.param_names:
        v = eng_b.view(name)
        v.copy_(rename(name).detach().to(eng_b.dtype).reshape(v.shape))


def test_product_of_two_rbf_factors_is_rbf_ard():
    from gdrf_amd.engine import Engine
    fac = [("kern0", "rbf", [0], 0.6, 2.0, None), ("kern1", "rbf", [1], 0.9, 1.5, None)]
    m, eps = prod_oracle(None, factors=fac, D=2)
    ep = engine_for(m)
    ea = Engine(m.N, m.M, m.K, m.V, 2, dtype=torch.float64, kernel="rbf", jitter=m.jitter, maxjitter=m.maxjitter, process_group=None, ard=True)
    ea.set_inducing_points(m.Z)
    ea.set_dirichlet(m.alpha)
    p = m.params
    _engine_pair(ea, lambda n: torch.stack([p["kern0.log_lengthscale"], p["kern1.log_lengthscale"]]) if n == "log_lengthscale"
                 else p["kern0.log_variance"] + p["kern1.log_variance"] if n == "log_variance" else p[n])
    xs, ws = dev(m.xs, ep), dev(m.ws, ep, torch.int32)
    for e in (ep, ea):
        e.loss_and_grads(xs, ws, dev(eps, e))
    assert abs(ep.read_out()["loss"] - ea.read_out()["loss"]) <= 1e-12 * abs(ea.read_out()["loss"])
    gp, ga = ep.named_views(ep.grads), ea.named_views(ea.grads)
    assert relerr(torch.stack([gp["kern0.log_lengthscale"], gp["kern1.log_lengthscale"]]).cpu(), ga["log_lengthscale"].cpu()) < 1e-9
    for n in ("kern0.log_variance", "kern1.log_variance"):
        assert relerr(gp[n].cpu(), ga["log_variance"].cpu()) < 1e-9
    for n in ("log_noise", "u_loc", "phi_unc", "u_scale_tril_unc"):
        assert relerr(gp[n].cpu(), ga[n].cpu()) < 1e-9, n


def test_product_of_two_periodic_factors_is_per_axis_periodic():
    from gdrf_amd.engine import Engine
    fac = [("kern0", "periodic", [0], 0.7, 2.0, 0.45), ("kern1", "periodic", [1], 1.1, 1.5, 0.6)]
    m, eps = prod_oracle(None, factors=fac, D=2)
    ep = engine_for(m)
    ea = Engine(m.N, m.M, m.K, m.V, 2, dtype=torch.float64, kernel="periodic", jitter=m.jitter, maxjitter=m.maxjitter, process_group=None,
                ard=True, period_count=2)
    ea.set_inducing_points(m.Z)
    ea.set_dirichlet(m.alpha)
    p = m.params
    pair = lambda leaf: torch.stack([p["kern0." + leaf], p["kern1." + leaf]])
    _engine_pair(ea, lambda n: pair(n) if n in ("log_lengthscale", "log_period")
                 else p["kern0.log_variance"] + p["kern1.log_variance"] if n == "log_variance" else p[n])
    xs, ws = dev(m.xs, ep), dev(m.ws, ep, torch.int32)
    for e in (ep, ea):
        e.loss_and_grads(xs, ws, dev(eps, e))
    assert abs(ep.read_out()["loss"] - ea.read_out()["loss"]) <= 1e-12 * abs(ea.read_out()["loss"])
    gp, ga = ep.named_views(ep.grads), ea.named_views(ea.grads)
    for leaf in ("log_lengthscale", "log_period"):
        assert relerr(torch.stack([gp["kern0." + leaf], gp["kern1." + leaf]]).cpu(), ga[leaf].cpu()) < 1e-9, leaf
    for n in ("kern0.log_variance", "kern1.log_variance"):
        assert relerr(gp[n].cpu(), ga["log_variance"].cpu()) < 1e-9


def test_five_adam_steps_fp64():
    m, _ = prod_oracle("rbf_ard01_periodic2_3d", optimizer="adam", lr=1e-2)
    eng = engine_for(m)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(5)
    for step in range(5):
        eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
        m.force_jitter_level = None
        loss_ref = m.step(eps)
        eng.loss_and_grads(xs, ws, dev(eps, eng), force_level=m.last_jitter_level)
        eng.adam("adam", 1e-2)
        assert abs(eng.read_out()["loss"] - loss_ref) / abs(loss_ref) < LOSS_TOL_VS_TORCH, step
    for name in eng.param_names:
        assert relerr(eng.view(name).cpu().numpy(), m.params[name].detach().numpy()) < 1e-8, name


def st_kernel(ls=(0.7, 1.1), period=0.45):
    from gdrf_amd.kernels import RBF, Periodic, Product
    return Product(RBF(2, active_dims=[0, 1], lengthscale=list(ls), variance=2.0), Periodic(1, active_dims=[2], lengthscale=0.8, period=period,
                                                                                         variance=1.5))


def _model(kernel, xs, ws, K=4, fixed=True, dtype=torch.float64):
    from gdrf_amd.models import SparseMultinomialGDRF
    D = xs.shape[1]
    return SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * D, kernel=kernel, num_observation_categories=ws.shape[1],
                                 num_topic_categories=K, dirichlet_param=0.01, n_points=list(NPTS[D]), fixed_inducing_points=fixed,
                                 inducing_init="grid" if fixed else "random", maxjitter=15, jitter=1e-6, device="cuda:0", dtype=dtype, seed=3)


@pytest.mark.parametrize("which", ["kern1.log_period", "kern0.log_variance"])
def test_changing_one_factor_parameter_refactorises(which):
    """A step behind the optimizer update factorises ahead (prefactorize); changing ONLY one factor's period or variance afterwards must be
    seen by the reuse check, or the next step would run on a stale L_uu."""
    m, _ = prod_oracle("rbf_ard01_periodic2_3d", lr=1e-2)
    model = _model(st_kernel(), m.xs.cuda(), m.ws.cuda())
    eng = model._engine_for(m.N)
    assert eng.prefactorize
    eng.set_inducing_points(m.Z)
    load(eng, m)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(7)
    for _ in range(2):
        eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
        m.step(eps)
        eng.loss_and_grads(xs, ws, dev(eps, eng)); eng.adam("adam", 1e-2)      # the second adam() factorises ahead
    new = m.params[which].detach().clone() + 0.2
    with torch.no_grad():
        m.params[which].copy_(new)
    sd = model.state_dict()
    key = {"kern1.log_period": "_kernel.kern1.period_unconstrained", "kern0.log_variance": "_kernel.kern0.variance_unconstrained"}[which]
    sd[key] = new.clone().cuda()
    model.load_state_dict(sd)
    eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
    eng.loss_and_grads(xs, ws, dev(eps, eng))
    m.force_jitter_level = eng.last_jitter_level
    loss_ref = float(m.loss(eps).detach())
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)


def test_unread_axis_gets_a_zero_inducing_gradient():
    """A lone Periodic on axis 1 of a 2-D world: the covariance ignores axis 0, so the learnable inducing inputs' axis-0 gradient is 0."""
    fac = [("", "periodic", [1], 0.8, 2.0, 0.4)]
    m, eps = prod_oracle(None, factors=fac, D=2, learn=True)
    eng = engine_for(m)
    assert set(eng.param_names) >= {"log_variance", "log_lengthscale", "log_period"}
    grads_ref = check_loss_and_grads(eng, m, eps)
    gz = eng.view("inducing_unc", eng.grads).cpu()
    assert torch.all(gz[:, 0] == 0) and torch.all(grads_ref["inducing_unc"][:, 0] == 0) and gz[:, 1].abs().max() > 0


def _svi(model, xs, opt="adam"):
    from gdrf_amd import poutine
    from gdrf_amd.infer import OBJECTIVE_DICT, SVI
    from gdrf_amd.optim import OPTIMIZER_DICT
    objective = OBJECTIVE_DICT["graphelbo"](max_plate_nesting=1, vectorize_particles=True, num_particles=1)
    scale = poutine.scale(scale=1.0 / len(xs))
    return SVI(model=scale(model.model), guide=scale(model.guide), optim=OPTIMIZER_DICT[opt]({"lr": 0.01}), loss=objective)


def _data(seed=3, V=20, K=4):
    xs, ws = inputs(3, seed=seed, W=30, H=20, V=V, K=K)
    return xs.cuda(), torch.as_tensor(ws).int().cuda()


def test_checkpoint_round_trip_and_growth(tmp_path):
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    from gdrf_amd.kernels import RBF, Periodic, Product
    xs, ws = _data()
    kern = Product(Product(RBF(1, active_dims=[0], lengthscale=0.6), RBF(1, active_dims=[1], lengthscale=0.8)),
                   Periodic(1, active_dims=[2], period=0.3, lengthscale=0.9))
    model = _model(kern, xs, ws, fixed=False)
    svi = _svi(model, xs, opt="rmsprop")
    losses = [svi.step(xs=xs[:200], ws=ws[:200], subsample=False) for _ in range(3)]
    assert all(np.isfinite(losses))
    sd = model.state_dict()
    assert {"_kernel.kern0.kern0.variance_unconstrained", "_kernel.kern0.kern1.lengthscale_unconstrained",
            "_kernel.kern1.period_unconstrained"} <= set(sd)
    assert "_kernel.variance_unconstrained" not in sd and "_kernel.lengthscale_unconstrained" not in sd
    kp = model.kernel_parameters
    assert set(kp) == {"kern0.kern0.variance", "kern0.kern0.lengthscale", "kern0.kern1.variance", "kern0.kern1.lengthscale",
                       "kern1.variance", "kern1.lengthscale", "kern1.period"}
    assert float(kp["kern1.period"]) != 0.3
    with pytest.raises(AttributeError):
        model.kernel_lengthscale
    with pytest.raises(AttributeError):
        model.kernel_variance
    st = svi.optim.get_state()
    assert "kern1.log_period" in st and "log_variance" not in st
    # growth keeps the parameters and the optimizer state
    e0 = model._engine
    p0, s0 = e0.params.clone(), e0.exp_avg_sq.clone()
    model._engine_for(2 * len(xs))
    assert model._engine is not e0 and torch.equal(model._engine.params, p0) and torch.equal(model._engine.exp_avg_sq, s0)
    assert np.isfinite(svi.step(xs=torch.cat([xs, xs]), ws=torch.cat([ws, ws]), subsample=False))
    snap = copy.deepcopy(model)
    torch.serialization.add_safe_globals([ModelSnapshot])
    torch.save({"model": snap}, tmp_path / "ckpt.pt")
    back = torch.load(tmp_path / "ckpt.pt", weights_only=True)["model"]
    assert torch.equal(back.topic_probs(xs), model.topic_probs(xs))
    re = back.restore(device="cuda:0")
    assert isinstance(re._kernel, Product) and re._kernel.active_dims == [0, 1, 2]
    assert re.state_dict().keys() == model.state_dict().keys()
    for k, v in re.kernel_parameters.items():
        assert np.array_equal(v, model.kernel_parameters[k]), k
    assert torch.equal(re.topic_probs(xs), model.topic_probs(xs))
    assert float(re.perplexity(xs, ws)) == float(model.perplexity(xs, ws))


def test_optim_args_callable_sees_the_factor_names():
    from gdrf_amd.optim import OPTIMIZER_DICT
    xs, ws = _data()
    model = _model(st_kernel(), xs, ws)
    seen = []

    def args(module_name, param_name):
        seen.append(param_name)
        return {"lr": 0.0 if param_name == "_kernel.kern1.period" else 0.01}
    from gdrf_amd import poutine
    from gdrf_amd.infer import OBJECTIVE_DICT, SVI
    scale = poutine.scale(scale=1.0 / len(xs))
    svi = SVI(model=scale(model.model), guide=scale(model.guide), optim=OPTIMIZER_DICT["adam"](args),
              loss=OBJECTIVE_DICT["graphelbo"](max_plate_nesting=1, vectorize_particles=True, num_particles=1))
    p0 = model.kernel_parameters
    for _ in range(2):
        svi.step(xs=xs, ws=ws, subsample=False)
    assert {"_kernel.kern0.variance", "_kernel.kern0.lengthscale", "_kernel.kern1.period"} <= set(seen)
    p1 = model.kernel_parameters
    assert float(p1["kern1.period"]) == float(p0["kern1.period"]) and float(p1["kern1.variance"]) != float(p0["kern1.variance"])


def _dist_build():
    xs, ws = _data()
    model = _model(st_kernel(), xs, ws)
    return model, _svi(model, xs), xs, ws


@pytest.mark.timeout(600)
def test_two_ranks_through_the_c_abi_hook_match_a_single_rank(tmp_path):
    r0, r1 = run_two_ranks(_dist_build, "c_abi_hook", 29700 + (os.getpid() % 2000), tmp_path)
    model, svi, xs, ws = _dist_build()
    ref = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(3)]
    assert r0["losses"] == r1["losses"]
    assert np.allclose(r0["losses"], ref, rtol=1e-10)
    assert torch.equal(r0["params"], r1["params"])
    assert (r0["params"] - model._engine.params.cpu()).abs().max() < 1e-9
