"""ARD kernels (one lengthscale per input dimension) on the GPU, against autograd through the reference-shaped CPU oracle, which
computes them by parameter substitution: a (D,) log-lengthscale broadcasts X / lengthscale exactly as pyro's Isotropy._scale does."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import RefShapedGDRF, conditional, synth_circles
from tests._util import (LOSS_TOL_VS_TORCH, NPTS, check_grads, check_loss_and_grads, dev, engine_for as ard_engine, relerr, run_two_ranks,
                         variant_oracle)

pytestmark = pytest.mark.gpu

LS = (0.12, 0.35, 0.2)
KINDS = ["rbf", "matern52", "matern32", "exponential", "rationalquadratic"]


def ard_oracle(kind="rbf", D=2, ls=LS, **kw):
    """The oracle of tests/_util.make_oracle with the (D,) lengthscale vector ``ls`` substituted for its scalar one."""
    def substitute(m):
        m.params["log_lengthscale"] = torch.tensor(ls[:D], dtype=m.dtype).log().requires_grad_(True)
    return variant_oracle(D, substitute, kind=kind, lengthscale=0.2, scale_mixture=1.3, shared_generator=True, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("learn,whiten", [(False, True), (True, True), (False, False)])
def test_loss_and_every_gradient_fp64(kind, D, learn, whiten):
    m, eps = ard_oracle(kind, D, learn=learn, whiten=whiten)
    eng = ard_engine(m)
    assert eng.view("log_lengthscale").shape == (D,) and eng.hyper_backward == "f64"
    # the tolerances of tests/test_gpu_parity.py::test_learnable_inducing_gradient_matches_autograd: the exponential kernel's 1/r in
    # dk/dr2, and points on a line (a badly conditioned K_uu), amplify the difference between the oracle's expanded-form distance and the
    # direct (x - z)^2 of the kernels (measured 1.4e-6 for the 1-D exponential case; test_equal_lengthscales_reproduce_the_isotropic_engine
    # holds the ARD form to the isotropic one there)
    tg = 1e-7
    if kind == "exponential":
        tg = 1e-6
    if D == 1 and (learn or kind == "exponential"):
        tg = 5e-6
    check_loss_and_grads(eng, m, eps, tg=tg)
    assert float(eng.grads[0]) == 0.0                     # slot 0 is not a parameter of an ARD context


def _iso_pair(kind="rbf", D=2, dtype=torch.float64, **kw):
    m, eps = ard_oracle(kind, D, ls=(0.2,) * D, dtype=dtype, **kw)
    eng_a = ard_engine(m)
    eng_i = ard_engine(m, ard=False)
    return m, eps, eng_a, eng_i


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [1, 2])
def test_equal_lengthscales_reproduce_the_isotropic_engine(kind, D):
    m, eps, eng_a, eng_i = _iso_pair(kind, D)
    xs, ws = dev(m.xs, eng_a), dev(m.ws, eng_a, torch.int32)
    for e in (eng_a, eng_i):
        e.loss_and_grads(xs, ws, dev(eps, e))
    la, li = eng_a.read_out()["loss"], eng_i.read_out()["loss"]
    assert abs(la - li) <= 1e-12 * abs(li)
    ga, gi = eng_a.named_views(eng_a.grads), eng_i.named_views(eng_i.grads)
    s = float(ga["log_lengthscale"].sum())
    assert abs(s - float(gi["log_lengthscale"])) <= 1e-9 * abs(float(gi["log_lengthscale"]))
    for name in gi:
        if name != "log_lengthscale":
            assert relerr(ga[name].cpu().numpy(), gi[name].cpu().numpy()) < 1e-9, name


def test_equal_lengthscales_fp32_f16x3_at_1e5_rows():
    from gdrf_amd.engine import Engine
    g = torch.Generator().manual_seed(3)
    N, K, V, D = 100_000, 6, 30, 2
    xs = torch.rand(N, D, generator=g)
    ws = torch.randint(0, 4, (N, V), generator=g, dtype=torch.int32)
    gx, gy = torch.meshgrid(torch.linspace(0, 1, 8), torch.linspace(0, 1, 6), indexing="ij")
    Z = torch.stack([gx.flatten(), gy.flatten()], 1)
    engs = []
    for ard in (True, False):
        e = Engine(N, Z.shape[0], K, V, D, dtype=torch.float32, kernel="matern52", jitter=1e-6, process_group=None, ard=ard)
        assert e.mfma_mode == "f16x3"
        e.set_inducing_points(Z)
        e.set_dirichlet(torch.full((K, V), 0.5, dtype=torch.float64))
        gp = torch.Generator().manual_seed(5)
        e.view("log_variance").fill_(np.log(4.0)); e.view("log_noise").fill_(0.1)
        e.view("u_loc").copy_(0.5 * torch.randn(K, Z.shape[0], generator=gp))
        e.view("phi_unc").copy_(0.3 * torch.randn(K, V, generator=gp))
        e.view("u_scale_tril_unc").copy_(0.05 * torch.randn(K, Z.shape[0], Z.shape[0], generator=gp).tril(-1) - 1.0 * torch.eye(Z.shape[0]))
        e.view("log_lengthscale").fill_(np.log(0.25))
        engs.append(e)
    eps = torch.randn(K, N, generator=g)
    out = []
    for e in engs:
        e.loss_and_grads(dev(xs, e), dev(ws, e, torch.int32), dev(eps, e))
        out.append((e.read_out()["loss"], e.named_views(e.grads)))
    (la, ga), (li, gi) = out
    assert abs(la - li) <= 5e-6 * abs(li)
    assert abs(float(ga["log_lengthscale"].double().sum()) - float(gi["log_lengthscale"])) <= 3e-3 * abs(float(gi["log_lengthscale"]))
    for name in gi:
        if name != "log_lengthscale":
            assert relerr(ga[name].cpu().numpy(), gi[name].cpu().numpy()) < 3e-3, name


@pytest.mark.parametrize("opt", ["adam", "adamw", "clippedadam"])
def test_five_optimizer_steps_fp64(opt):
    m, _ = ard_oracle("matern32", 2, optimizer=opt, lr=1e-2)
    eng = ard_engine(m)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(5)
    for step in range(5):
        eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
        loss_ref = m.step(eps)
        eng.loss_and_grads(xs, ws, dev(eps, eng))
        eng.adam(opt, 1e-2, weight_decay=0.01 if opt == "adamw" else 0.0)
        out = eng.read_out()
        assert abs(out["loss"] - loss_ref) / abs(loss_ref) < LOSS_TOL_VS_TORCH, (step, out, loss_ref)
    for name in eng.param_names:
        assert relerr(eng.view(name).cpu().numpy(), m.params[name].detach().numpy()) < 1e-8, name
    assert float(eng.params[0]) == 0.0


@pytest.mark.parametrize("how", ["load_state_dict", "view"])
def test_changing_one_axis_lengthscale_refactorises(how):
    """A step behind the optimizer update factorises ahead on the parameters it just wrote (prefactorize); changing ONLY one per-axis
    lengthscale afterwards must be seen by the reuse check, or the next step would run on a stale L_uu."""
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    m, _ = ard_oracle("rbf", 2, lr=1e-2)
    model = SparseMultinomialGDRF(xs=m.xs.cuda(), ws=m.ws.cuda(), world=[(0.0, 1.0)] * 2, kernel=RBF(2, lengthscale=list(LS[:2]), variance=25.0),
                                  num_observation_categories=m.V, num_topic_categories=m.K, dirichlet_param=0.01, n_points=list(NPTS[2]),
                                  fixed_inducing_points=True, inducing_init="grid", maxjitter=15, jitter=1e-6, device="cuda:0", dtype=torch.float64)
    eng = model._engine_for(m.N)
    assert eng.ard and eng.prefactorize
    eng.set_inducing_points(m.Z)
    for name in eng.param_names:
        eng.view(name).copy_(m.params[name].detach().to(eng.device))
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(7)
    for _ in range(2):
        eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
        m.step(eps)
        eng.loss_and_grads(xs, ws, dev(eps, eng)); eng.adam("adam", 1e-2)      # the second adam() factorises ahead
    new = m.params["log_lengthscale"].detach().clone()
    new[1] += 0.3
    with torch.no_grad():
        m.params["log_lengthscale"].copy_(new)
    if how == "load_state_dict":
        sd = model.state_dict()
        sd["_kernel.lengthscale_unconstrained"] = new.clone()
        model.load_state_dict(sd)
    else:
        eng.view("log_lengthscale")[1] = float(new[1])
    eps = torch.randn(m.K, m.N, generator=g, dtype=torch.float64)
    eng.loss_and_grads(xs, ws, dev(eps, eng))
    m.force_jitter_level = eng.last_jitter_level
    loss_ref = float(m.loss(eps).detach())
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)


@pytest.mark.parametrize("kind", ["rbf", "matern52", "rationalquadratic"])
@pytest.mark.parametrize("D", [2, 3])
def test_predictive_path(kind, D):
    m, _ = ard_oracle(kind, D, W=23, H=11, V=9, K=5)
    eng = ard_engine(m)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    lvl = eng.factorize()
    m.force_jitter_level = lvl
    assert relerr(eng.predict(xs, 0).cpu().numpy(), m.log_topic_probs().detach().numpy()) < 1e-9
    assert relerr(eng.predict(xs, 1).cpu().numpy(), m.topic_probs().detach().numpy()) < 1e-9
    assert relerr(eng.predict(xs, 2).cpu().numpy(), m.word_probs().detach().numpy()) < 1e-9
    s = eng.predict(xs, 3, ws).cpu().numpy()
    perp = float(np.exp(-s[0] / s[1]))
    assert abs(perp - float(m.perplexity())) / float(m.perplexity()) < 1e-9
    c = m.constrained()
    with torch.no_grad():
        loc, var = conditional(kind, m.xs, m.inducing(), c["lengthscale"], c["variance"], c["u_loc"], c["u_scale_tril"], m._luu(c),
                               c["scale_mixture"], whiten=True)
    lv = eng.predict(xs, 4).cpu()
    assert relerr(lv[0].numpy(), loc.numpy()) < 1e-9 and relerr(lv[1].numpy(), var.numpy()) < 1e-9


def test_knm_entry_point():
    from oracle.gdrf_oracle import kernel_matrix
    m, _ = ard_oracle("matern52", 3)
    eng = ard_engine(m)
    c = m.constrained()
    ref = kernel_matrix("matern52", m.xs, m.Z, c["lengthscale"].detach(), c["variance"].detach())
    assert relerr(eng.knm(dev(m.xs, eng)).cpu().numpy(), ref.numpy()) < 1e-12


def _model(ls=(0.15, 0.3), dtype=torch.float64, K=4, V=20, seed=3, device="cuda:0", fixed=True, kernel="rbf"):
    from gdrf_amd.kernels import KERNEL_DICT
    from gdrf_amd.models import SparseMultinomialGDRF
    xs_np, ws_np, _ = synth_circles(30, 20, V, K, seed=seed)
    xs = torch.from_numpy(xs_np).float().to(device)
    ws = torch.from_numpy(ws_np).int().to(device)
    world = list(zip(xs.min(dim=0).values.cpu().numpy().tolist(), xs.max(dim=0).values.cpu().numpy().tolist()))
    model = SparseMultinomialGDRF(xs=xs, ws=ws, world=world, kernel=KERNEL_DICT[kernel](input_dim=2, lengthscale=list(ls), variance=25.0),
                                  num_observation_categories=V, num_topic_categories=K, dirichlet_param=0.01, n_points=[6, 5],
                                  fixed_inducing_points=fixed, inducing_init="grid" if fixed else "random", maxjitter=15, jitter=1e-6,
                                  device=device, dtype=dtype, seed=seed)
    return model, xs, ws


def _build(dtype=torch.float64, device="cuda:0", opt="adamw", loss="graphelbo", particles=1):
    from gdrf_amd import poutine
    from gdrf_amd.infer import OBJECTIVE_DICT, SVI
    from gdrf_amd.optim import OPTIMIZER_DICT
    model, xs, ws = _model(dtype=dtype, device=device)
    optimizer = OPTIMIZER_DICT[opt]({"lr": 0.01})
    objective = OBJECTIVE_DICT[loss](max_plate_nesting=1, vectorize_particles=True, num_particles=particles)
    scale = poutine.scale(scale=1.0 / len(xs))
    svi = SVI(model=scale(model.model), guide=scale(model.guide), optim=optimizer, loss=objective)
    return model, svi, optimizer, xs, ws


def test_surface_and_checkpoint(tmp_path):
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    model, svi, optimizer, xs, ws = _build()
    for _ in range(3):
        svi.step(xs=xs, ws=ws, subsample=False)
    sd = model.state_dict()
    assert sd["_kernel.lengthscale_unconstrained"].shape == (2,)
    ls = model.kernel_lengthscale
    assert ls.shape == (2,) and np.allclose(ls, sd["_kernel.lengthscale_unconstrained"].exp().cpu().numpy())
    assert np.array_equal(model.artifacts(xs, ws)["kernel lengthscale"], ls)
    bad = dict(sd); bad["_kernel.lengthscale_unconstrained"] = torch.zeros(())
    with pytest.raises(RuntimeError):
        model.load_state_dict(bad)
    snap = copy.deepcopy(model)
    torch.serialization.add_safe_globals([ModelSnapshot])
    torch.save({"model": snap}, tmp_path / "ckpt.pt")
    back = torch.load(tmp_path / "ckpt.pt", weights_only=True)["model"]
    re = back.restore()
    assert re._kernel.ard and re._engine.ard
    assert torch.equal(back.topic_probs(xs), model.topic_probs(xs))
    st = optimizer.get_state()
    assert any(tuple(v.shape) == (2,) for v in _tensors(st))
    model2, svi2, opt2, _, _ = _build()
    model2.load_state_dict(sd)
    svi2.step(xs=xs, ws=ws, subsample=False)              # binds the optimizer to the engine
    opt2.set_state(st)
    assert all(torch.equal(a, b) for a, b in zip(_tensors(opt2.get_state()), _tensors(st)))


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _tensors(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _tensors(v)


def test_engine_growth_keeps_ard():
    model, svi, _, xs, ws = _build()
    svi.step(xs=xs[:50], ws=ws[:50], subsample=False)
    e0 = model._engine
    big = torch.cat([xs, xs]); bigw = torch.cat([ws, ws])
    model._engine_for(len(big))
    assert model._engine is not e0 and model._engine.ard and model.kernel_lengthscale.shape == (2,)
    assert np.isfinite(svi.step(xs=big, ws=bigw, subsample=False))


def test_non_unit_world_against_the_oracle():
    world = [(-3.0, 5.0), (10.0, 12.0)]
    xs, ws, _ = synth_circles(17, 11, 9, 3, seed=4)
    lower = torch.tensor([w[0] for w in world], dtype=torch.float64)
    delta = torch.tensor([w[1] - w[0] for w in world], dtype=torch.float64)
    xs_w = torch.from_numpy(xs).double() * delta + lower
    m = RefShapedGDRF(xs_w, ws, kind="matern52", K=3, n_points=(5, 4), lengthscale=0.3, jitter=1e-6, world=world)
    m.params["log_lengthscale"] = torch.tensor([0.2, 0.45], dtype=torch.float64).log().requires_grad_(True)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        m.params["u_loc"].add_(0.3 * torch.randn(m.params["u_loc"].shape, generator=g, dtype=torch.float64))
    eps = torch.randn(3, m.N, generator=g, dtype=torch.float64)
    loss_ref, grads_ref = m.loss_and_grads(eps)
    eng = ard_engine(m)
    xs_m = m.scale(xs_w)
    eng.loss_and_grads(dev(xs_m, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), xs_guide=dev(m.scale(xs_m), eng),
                       force_level=m.last_jitter_level)
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)
    check_grads(eng, grads_ref)


def test_particles_and_renyi():
    m, _ = ard_oracle("matern32", 2)
    eng = ard_engine(m)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    g = torch.Generator().manual_seed(11)
    eps3 = torch.randn(3, m.K, m.N, generator=g, dtype=torch.float64)
    # Trace_ELBO, 3 particles: the mean of the single-particle estimates
    eng.loss_and_grads(xs, ws, dev(eps3, eng))
    l3, g3 = eng.read_out()["loss"], eng.grads.clone()
    ls, gs = [], []
    for p in range(3):
        eng.loss_and_grads(xs, ws, dev(eps3[p], eng))
        ls.append(eng.read_out()["loss"]); gs.append(eng.grads.clone())
    assert abs(l3 - np.mean(ls)) <= 1e-12 * abs(l3)
    assert relerr(g3.cpu().numpy(), torch.stack(gs).mean(0).cpu().numpy()) < 1e-12
    # RenyiELBO(alpha = 0.5, 3 particles) against the oracle
    eng.loss_and_grads(xs, ws, dev(eps3, eng), renyi_alpha=0.5)
    m.force_jitter_level = eng.last_jitter_level
    loss_ref, grads_ref = m.loss_and_grads(eps3, renyi_alpha=0.5)
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)
    check_grads(eng, grads_ref)


def test_streaming_minibatch_with_n_global():
    m, eps = ard_oracle("rbf", 2)
    eng = ard_engine(m)
    idx = torch.arange(0, m.N, 3)
    xs_b, ws_b, eps_b = m.xs[idx], m.ws[idx], eps[:, idx]
    eng.loss_and_grads(dev(xs_b, eng), dev(ws_b, eng, torch.int32), dev(eps_b, eng), n_global=m.N)
    m.force_jitter_level = eng.last_jitter_level
    loss_ref, grads_ref = m.loss_and_grads(eps_b, xs=xs_b, ws=ws_b, n_global=m.N)
    assert abs(eng.read_out()["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref)
    check_grads(eng, grads_ref)


def test_mean_function_and_custom_link():
    mf = lambda x: 1.5 * x[:, 0] - 0.7 * x[:, 1]
    link = lambda mu: torch.softmax(2.0 * mu, -2)
    m, eps = ard_oracle("matern52", 2, mean_function=mf, link_function=link)
    eng = ard_engine(m)
    eng.link_function = link
    check_loss_and_grads(eng, m, eps, mean=dev(mf(m.xs), eng))
    assert float(eng.grads[0]) == 0.0


def test_hyper_backward_tn_request_falls_back_to_f64():
    m, eps = ard_oracle("rbf", 2, dtype=torch.float32)
    e_tn = ard_engine(m, hyper_backward="tn")
    e_64 = ard_engine(m, hyper_backward="f64")
    assert e_tn.hyper_backward == "f64" and e_tn.mfma_mode == "f16x3"
    xs, ws = dev(m.xs, e_tn), dev(m.ws, e_tn, torch.int32)
    for e in (e_tn, e_64):
        e.loss_and_grads(xs, ws, dev(eps, e))
    assert e_tn.read_out()["loss"] == e_64.read_out()["loss"]
    assert torch.equal(e_tn.grads, e_64.grads)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("via", ["torch_distributed", "c_abi_hook"])
def test_two_ranks_on_one_gpu_match_a_single_rank(tmp_path, via):
    port = 27600 + (os.getpid() % 2000) + (7 if via == "c_abi_hook" else 0)
    r0, r1 = run_two_ranks(_build, via, port, tmp_path)
    model, svi, _, xs, ws = _build(dtype=torch.float64)
    ref = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(3)]
    assert r0["losses"] == r1["losses"]
    assert np.allclose(r0["losses"], ref, rtol=1e-10)
    assert torch.equal(r0["params"], r1["params"])
    assert (r0["params"] - model._engine.params.cpu()).abs().max() < 1e-9
