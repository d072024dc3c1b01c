"""The Periodic kernel on the GPU, against autograd through the reference-shaped CPU oracle with pyro's sine form of the kernel
(pyro 1.8.0 contrib/gp/kernels/periodic.py):

    k(x, z) = variance * exp(-2 sum_d sin^2(pi (x_d - z_d) / period_d) / lengthscale_d^2),   k(x, x) = variance

The oracle is RefShapedGDRF with kind "periodic" (oracle/gdrf_oracle.py::periodic_matrix)."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import oracle.gdrf_oracle as go
from oracle.gdrf_oracle import RefShapedGDRF, periodic_matrix, synth_circles
from tests._util import (LOSS_TOL_VS_TORCH, NPTS, check_grads, check_loss_and_grads, dev, engine_for as per_engine, relerr, run_two_ranks,
                         variant_oracle)

pytestmark = pytest.mark.gpu

LS = {1: (0.8,), 2: (0.7, 1.1)}
PER = {1: (0.37,), 2: (0.45, 0.6)}


def with_periodic_params(m, lengthscale, period):
    """``m`` (built with a scalar lengthscale and period) with log-lengthscale and log-period of shape () or (D,) substituted."""
    for name, value in (("log_lengthscale", lengthscale), ("log_period", period)):
        m.params[name] = torch.as_tensor(value, dtype=m.dtype).log().clone().requires_grad_(True)
    return m


def periodic_ref(xs, ws, *, period, lengthscale, **kw):
    return with_periodic_params(RefShapedGDRF(xs, ws, kind="periodic", period=float(torch.as_tensor(period).flatten()[0]), **kw),
                                lengthscale, period)


def per_oracle(D=1, per_axis=False, ls=None, period=None, **kw):
    ls = LS[D] if ls is None else ls
    period = PER[D] if period is None else period
    if not per_axis:
        ls, period = ls[0], period[0]
    return variant_oracle(D, lambda m: with_periodic_params(m, ls, period), kind="periodic", variance=4.0,
                          period=float(torch.as_tensor(period).flatten()[0]), **kw)


CASES = [(1, False), (2, False), (2, True)]        # (D, per-axis lengthscale and period); one element is the shared form at D = 1


@pytest.mark.parametrize("D,per_axis", CASES)
@pytest.mark.parametrize("learn,whiten", [(False, True), (True, True), (False, False)])
def test_loss_and_every_gradient_fp64(D, per_axis, learn, whiten):
    m, eps = per_oracle(D, per_axis, learn=learn, whiten=whiten)
    eng = per_engine(m)
    assert eng.view("log_period").shape == ((D,) if per_axis else ()) and eng.hyper_backward == "f64"
    check_loss_and_grads(eng, m, eps)


@pytest.mark.parametrize("ls,period", [(0.8, PER[2]), (LS[2], 0.4)])
def test_mixed_shapes_of_lengthscale_and_period(ls, period):
    m, eps = per_oracle(2, per_axis=True, ls=ls, period=period)
    eng = per_engine(m)
    assert eng.view("log_lengthscale").shape == torch.as_tensor(ls).shape and eng.view("log_period").shape == torch.as_tensor(period).shape
    check_loss_and_grads(eng, m, eps)


@pytest.mark.parametrize("D", [1, 2])
def test_knm_against_the_sine_form(D):
    m, _ = per_oracle(D, per_axis=True)
    c = m.constrained()
    ref = periodic_matrix(m.xs, m.Z, c["lengthscale"].detach(), c["variance"].detach(), c["kernel_kw"]["period"].detach()).numpy()
    e64 = per_engine(m)
    assert relerr(e64.knm(dev(m.xs, e64)).cpu().numpy(), ref) < 1e-12
    e32 = per_engine(m, dtype=torch.float32)
    assert relerr(e32.knm(dev(m.xs, e32)).cpu().numpy(), ref) < 2e-6
    big = per_engine(m, n_cap=16)          # more rows than the context holds: gdrf_knm grows its scratch
    assert relerr(big.knm(dev(m.xs, big)).cpu().numpy(), ref) < 1e-12


def test_shifting_every_row_by_one_period_leaves_knm_unchanged():
    g = torch.Generator().manual_seed(2)
    m, _ = per_oracle(1, period=(0.25,))
    eng = per_engine(m)
    xs = 0.75 * torch.rand(500, 1, generator=g, dtype=torch.float64)
    k0 = eng.knm(dev(xs, eng)).cpu().numpy()
    k1 = eng.knm(dev(xs + 0.25, eng)).cpu().numpy()
    assert relerr(k1, k0) < 1e-13
    assert relerr(k0, eng.knm(dev(xs + 0.1, eng)).cpu().numpy()) > 1e-3


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-9), (torch.float32, 5e-4)])
def test_predictive_path(D, dtype, tol):
    from gdrf_amd.kernels import Periodic
    m, _ = per_oracle(D, per_axis=D == 2, W=23, H=11, V=9, K=5)
    eng = per_engine(m, dtype=dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    m.force_jitter_level = eng.factorize()
    assert relerr(eng.predict(xs, 0).cpu().numpy(), m.log_topic_probs().detach().numpy()) < tol
    assert relerr(eng.predict(xs, 1).cpu().numpy(), m.topic_probs().detach().numpy()) < tol
    assert relerr(eng.predict(xs, 2).cpu().numpy(), m.word_probs().detach().numpy()) < tol
    s = eng.predict(xs, 3, ws).cpu().double().numpy()
    assert abs(float(np.exp(-s[0] / s[1])) - float(m.perplexity())) / float(m.perplexity()) < tol
    c = m.constrained()
    with torch.no_grad():
        loc, var = go.conditional("periodic", m.xs, m.inducing(), c["lengthscale"], c["variance"], c["u_loc"], c["u_scale_tril"],
                                  m._luu(c), whiten=True, **c["kernel_kw"])
    lv = eng.predict(xs, 4).cpu()
    assert relerr(lv[0].numpy(), loc.numpy()) < tol and relerr(lv[1].numpy(), var.numpy()) < tol
    # model.forward(xs): the same conditional through the public surface
    from gdrf_amd.models import SparseMultinomialGDRF
    kern = Periodic(D, lengthscale=list(LS[D][:D]) if D == 2 else LS[1][0], period=list(PER[D]) if D == 2 else PER[1][0], variance=4.0)
    model = SparseMultinomialGDRF(xs=m.xs.to(dtype).cuda(), ws=m.ws.cuda(), world=[(0.0, 1.0)] * D, kernel=kern, num_observation_categories=m.V,
                                  num_topic_categories=m.K, dirichlet_param=0.01, n_points=list(NPTS[D]), fixed_inducing_points=True,
                                  inducing_init="grid", maxjitter=15, jitter=1e-6, device="cuda:0", dtype=dtype)
    me = model._engine_for(m.N)
    me.set_inducing_points(m.Z)
    for name in me.param_names:
        me.view(name).copy_(m.params[name].detach().to(me.dtype).reshape(me.view(name).shape))
    f_loc, f_var = model.forward(m.xs.to(dtype).cuda())
    assert relerr(f_loc.cpu().numpy(), loc.numpy()) < tol and relerr(f_var.cpu().numpy(), var.numpy()) < tol


def test_five_adam_steps_fp64():
    m, _ = per_oracle(2, per_axis=True, optimizer="adam", lr=1e-2)
    eng = per_engine(m)
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


def test_five_rmsprop_steps_fp64():
    from gdrf_amd.optim import OPTIMIZER_DICT
    m, _ = per_oracle(1)
    eng = per_engine(m)
    o = OPTIMIZER_DICT["rmsprop"]({"lr": 1e-2})
    o._bind(eng)
    ref = {n: torch.optim.RMSprop([p], foreach=False, **o.args_for(n)) for n, p in m.params.items()}
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(6)
    for step in range(5):
        eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
        m.force_jitter_level = None
        loss_ref, _ = m.loss_and_grads(eps)
        for opt in ref.values():
            opt.step()
        eng.loss_and_grads(xs, ws, dev(eps, eng), force_level=m.last_jitter_level)
        o._step()
        assert abs(eng.read_out()["loss"] - loss_ref) / abs(loss_ref) < LOSS_TOL_VS_TORCH, step
    for name in eng.param_names:
        assert relerr(eng.view(name).cpu().numpy(), m.params[name].detach().numpy()) < 1e-8, name


def _model(D=1, dtype=torch.float64, K=4, V=20, seed=3, device="cuda:0", fixed=True, period=None, ls=None, rows_form="auto",
           mean_function=None, world=None, xs=None, ws=None):
    from gdrf_amd.kernels import Periodic
    from gdrf_amd.models import SparseMultinomialGDRF
    if xs is None:
        xs_np, ws_np, _ = synth_circles(30, 20, V, K, seed=seed, one_d=(D == 1))
        xs = torch.from_numpy(xs_np).to(dtype).to(device)
        ws = torch.from_numpy(ws_np).int().to(device)
    world = world or [(0.0, 1.0)] * D
    kern = Periodic(D, lengthscale=ls or 0.8, period=period or 0.3, variance=4.0)
    model = SparseMultinomialGDRF(xs=xs, ws=ws, world=world, kernel=kern, num_observation_categories=V, num_topic_categories=K,
                                  dirichlet_param=0.01, n_points=list(NPTS[D]), fixed_inducing_points=fixed,
                                  inducing_init="grid" if fixed else "random", maxjitter=15, jitter=1e-6, device=device, dtype=dtype,
                                  seed=seed, rows_form=rows_form, mean_function=mean_function)
    return model, xs, ws


def _build(dtype=torch.float64, opt="adam", loss="graphelbo", particles=1, **kw):
    from gdrf_amd import poutine
    from gdrf_amd.infer import OBJECTIVE_DICT, SVI
    from gdrf_amd.optim import OPTIMIZER_DICT
    model, xs, ws = _model(dtype=dtype, **kw)
    optimizer = OPTIMIZER_DICT[opt]({"lr": 0.01})
    objective = OBJECTIVE_DICT[loss](max_plate_nesting=1, vectorize_particles=True, num_particles=particles)
    scale = poutine.scale(scale=1.0 / len(xs))
    svi = SVI(model=scale(model.model), guide=scale(model.guide), optim=optimizer, loss=objective)
    return model, svi, optimizer, xs, ws


@pytest.mark.parametrize("how", ["load_state_dict", "view"])
def test_changing_only_the_period_refactorises(how):
    """A step behind the optimizer update factorises ahead on the parameters it just wrote (prefactorize); changing ONLY the period
    afterwards must be seen by the reuse check, or the next step would run on a stale L_uu."""
    m, _ = per_oracle(1, lr=1e-2)
    model, _, _ = _model(1, xs=m.xs.cuda(), ws=m.ws.cuda(), period=PER[1][0], ls=LS[1][0])
    eng = model._engine_for(m.N)
    assert eng.prefactorize
    eng.set_inducing_points(m.Z)
    for name in eng.param_names:
        eng.view(name).copy_(m.params[name].detach().to(eng.device).reshape(eng.view(name).shape))
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(7)
    for _ in range(2):
        eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
        m.step(eps)
        eng.loss_and_grads(xs, ws, dev(eps, eng)); eng.adam("adam", 1e-2)      # the second adam() factorises ahead
    new = m.params["log_period"].detach().clone() + 0.2
    with torch.no_grad():
        m.params["log_period"].copy_(new)
    if how == "load_state_dict":
        sd = model.state_dict()
        sd["_kernel.period_unconstrained"] = new.clone().cuda()
        model.load_state_dict(sd)
    else:
        eng.view("log_period").fill_(float(new))
    eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
    eng.loss_and_grads(xs, ws, dev(eps, eng))
    m.force_jitter_level = eng.last_jitter_level
    loss_ref = float(m.loss(eps).detach())
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)


def test_non_unit_world_against_the_oracle():
    world = [(-3.0, 5.0), (10.0, 12.0)]
    xs, ws, _ = synth_circles(17, 11, 9, 3, seed=4)
    lower = torch.tensor([w[0] for w in world], dtype=torch.float64)
    delta = torch.tensor([w[1] - w[0] for w in world], dtype=torch.float64)
    xs_w = torch.from_numpy(xs).double() * delta + lower
    m = periodic_ref(xs_w, ws, K=3, n_points=(5, 4), jitter=1e-6, world=world, variance=4.0, lengthscale=(0.6, 0.9), period=(0.5, 0.7))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        m.params["u_loc"].add_(0.3 * torch.randn(m.params["u_loc"].shape, generator=g, dtype=torch.float64))
    eps = torch.randn(3, m.N, generator=g, dtype=torch.float64)
    loss_ref, grads_ref = m.loss_and_grads(eps)
    eng = per_engine(m)
    xs_m = m.scale(xs_w)
    eng.loss_and_grads(dev(xs_m, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), xs_guide=dev(m.scale(xs_m), eng),
                       force_level=m.last_jitter_level)
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)
    check_grads(eng, grads_ref)


def test_streamed_rows_form():
    m, eps = per_oracle(2, per_axis=True)
    eng = per_engine(m, rows_form="streamed")
    assert eng.rows_form == "streamed"
    check_loss_and_grads(eng, m, eps)


def test_two_particles_renyi():
    m, _ = per_oracle(1)
    eng = per_engine(m)
    g = torch.Generator().manual_seed(11)
    eps2 = torch.randn(2, m.K, m.N, generator=g, dtype=torch.float64)
    eng.loss_and_grads(dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps2, eng), renyi_alpha=0.5)
    m.force_jitter_level = eng.last_jitter_level
    loss_ref, grads_ref = m.loss_and_grads(eps2, renyi_alpha=0.5)
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)
    check_grads(eng, grads_ref)


def test_mean_function():
    mf = lambda x: 1.5 * torch.cos(6.0 * x[:, 0])
    m, eps = per_oracle(1, mean_function=mf)
    eng = per_engine(m)
    check_loss_and_grads(eng, m, eps, mean=dev(mf(m.xs), eng))


def test_mean_function_module_trains_beside_the_period():
    class Mean(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.tensor(0.5, dtype=torch.float64, device="cuda:0"))

        def forward(self, x):
            return self.a * torch.cos(6.0 * x[:, 0])
    model, svi, _, xs, ws = _build(mean_function=Mean())
    a0, p0 = float(model._mean_function.a), float(model.kernel_period)
    for _ in range(3):
        assert np.isfinite(svi.step(xs=xs, ws=ws, subsample=False))
    assert float(model._mean_function.a) != a0 and float(model.kernel_period) != p0


@pytest.mark.timeout(600)
def test_two_ranks_through_the_c_abi_hook_match_a_single_rank(tmp_path):
    r0, r1 = run_two_ranks(_build, "c_abi_hook", 28700 + (os.getpid() % 2000), tmp_path)
    model, svi, _, xs, ws = _build(dtype=torch.float64)
    ref = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(3)]
    assert r0["losses"] == r1["losses"]
    assert np.allclose(r0["losses"], ref, rtol=1e-10)
    assert torch.equal(r0["params"], r1["params"])
    lp = model._engine.layout["log_period"]
    assert abs(float(r0["params"][lp]) - float(model._engine.params[lp])) < 1e-9
    assert (r0["params"] - model._engine.params.cpu()).abs().max() < 1e-9


def test_seasonal_dataset_trains_and_checkpoints(tmp_path):
    """1-D synthetic seasonal record: topic weights follow sin(2 pi t / 0.25).  SVI.step with svi.optim, then a torch.save /
    weights_only round trip of the model gives identical predictions."""
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    g = torch.Generator().manual_seed(0)
    N, V, K = 2000, 12, 2
    t = torch.rand(N, 1, generator=g, dtype=torch.float64)
    w = 0.5 + 0.5 * torch.sin(2 * math.pi * t[:, 0] / 0.25)
    phi = torch.softmax(3.0 * torch.randn(K, V, generator=g, dtype=torch.float64), -1)
    probs = w[:, None] * phi[0] + (1 - w[:, None]) * phi[1]
    ws = torch.stack([torch.multinomial(p, 20, replacement=True, generator=g).bincount(minlength=V) for p in probs]).int()
    model, svi, optimizer, xs, ws = _build(K=K, V=V, xs=t.cuda(), ws=ws.cuda(), period=0.3, opt="adam")
    losses = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(30)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert svi.optim is optimizer
    assert model.kernel_period.shape == () and float(model.kernel_period) != 0.3
    sd = model.state_dict()
    assert sd["_kernel.period_unconstrained"].shape == ()
    assert "kernel lengthscale" in model.artifacts(xs, ws)
    snap = copy.deepcopy(model)
    torch.serialization.add_safe_globals([ModelSnapshot])
    torch.save({"model": snap}, tmp_path / "ckpt.pt")
    back = torch.load(tmp_path / "ckpt.pt", weights_only=True)["model"]
    assert torch.equal(back.topic_probs(xs), model.topic_probs(xs))
    re = back.restore(device="cuda:0")
    assert re._kernel.name == "periodic" and float(re.kernel_period) == float(model.kernel_period)
    assert torch.equal(re.topic_probs(xs), model.topic_probs(xs))
    assert torch.equal(re.word_probs(xs), model.word_probs(xs))
    assert float(re.perplexity(xs, ws)) == float(model.perplexity(xs, ws))


def test_per_axis_period_checkpoint_and_growth():
    model, svi, _, xs, ws = _build(opt="rmsprop")
    svi.step(xs=xs[:50], ws=ws[:50], subsample=False)
    e0 = model._engine
    model._engine_for(2 * len(xs))
    assert model._engine is not e0 and "log_period" in model._engine.param_names
    assert np.isfinite(svi.step(xs=torch.cat([xs, xs]), ws=torch.cat([ws, ws]), subsample=False))
    from gdrf_amd.kernels import Periodic
    from gdrf_amd.models import SparseMultinomialGDRF
    xs_np, ws_np, _ = synth_circles(12, 10, 8, 3, seed=1)
    m2 = SparseMultinomialGDRF(xs=torch.from_numpy(xs_np).cuda(), ws=torch.from_numpy(ws_np).int().cuda(), world=[(0.0, 1.0)] * 2,
                               kernel=Periodic(2, lengthscale=[0.6, 0.9], period=[0.4, 0.7]), num_observation_categories=8,
                               num_topic_categories=3, dirichlet_param=0.01, n_points=[3, 3], device="cuda:0")
    sd = m2.state_dict()
    assert sd["_kernel.period_unconstrained"].shape == (2,) and sd["_kernel.lengthscale_unconstrained"].shape == (2,)
    assert np.allclose(m2.kernel_period, [0.4, 0.7])
    re = copy.deepcopy(m2).restore()
    assert re.kernel_period.shape == (2,) and np.allclose(re.kernel_period, [0.4, 0.7])
