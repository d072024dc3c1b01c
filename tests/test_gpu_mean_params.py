"""Trainable parameters of a torch.nn.Module mean_function on the GPU: the gradient of the engine's mean segment and the loss of
SVI.step against torch.autograd through the reference-shaped oracle (which differentiates through the same module), the optimizer
trajectory against torch optimizers on the module, the unchanged data path of plain callables, two ranks, and checkpoints."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import RefShapedGDRF, _ClippedAdam, synth_circles
from tests._util import LOSS_TOL_VS_TORCH, perturb_posterior, run_two_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, V, NPTS = 4, 12, (4, 3)
WORLD = [(2.0, 5.0), (-1.0, 3.0)]
SIGMOID_LINK = lambda mu: 0.05 + torch.sigmoid(0.02 * mu)       # noqa: E731  (not shift-invariant over the topics, unlike softmax)


class Const(torch.nn.Module):
    """A learnt prior prevalence per topic: (K, 1)."""

    def __init__(self, g):
        super().__init__()
        self.c = torch.nn.Parameter(torch.randn(K, 1, generator=g, dtype=torch.float64))

    def forward(self, x):
        return self.c


class TrendKN(torch.nn.Module):
    """A linear trend per topic: (K, D+1) weights, (K, n) values."""

    def __init__(self, g, D=2):
        super().__init__()
        self.w = torch.nn.Parameter(0.8 * torch.randn(K, D + 1, generator=g, dtype=torch.float64))

    def forward(self, x):
        x = x.to(self.w.dtype)
        return self.w[:, :-1] @ x.T + self.w[:, -1:]


class TrendN(torch.nn.Module):
    """One trend shared by the topics: (D+1,) weights, (n,) values."""

    def __init__(self, g, D=2):
        super().__init__()
        self.w = torch.nn.Parameter(0.8 * torch.randn(D + 1, generator=g, dtype=torch.float64))

    def forward(self, x):
        x = x.to(self.w.dtype)
        return x @ self.w[:-1] + self.w[-1]


MEANS = {"const": Const, "trend_kn": TrendKN, "trend_n": TrendN}


def relerr(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-300))


def setup(mean="trend_kn", dtype=torch.float64, whiten=True, learn=False, ard=False, world=False, link=None, P=1, renyi=None,
          opt="adam", lr=1e-2, seed=3):
    """(oracle, model, svi, eps, xs, ws, reference module): the model holds exactly the oracle's parameters; the oracle's mean is a
    CPU copy of the model's module."""
    from gdrf_amd import poutine
    from gdrf_amd.infer import SVI, RenyiELBO, Trace_ELBO
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    from gdrf_amd.optim import OPTIMIZER_DICT
    xs, ws, _ = synth_circles(15, 11, V, K, seed=seed)
    xs = torch.from_numpy(xs).double()
    g = torch.Generator().manual_seed(seed + 100)
    if world:
        lower = torch.tensor([w[0] for w in WORLD], dtype=torch.float64)
        delta = torch.tensor([w[1] - w[0] for w in WORLD], dtype=torch.float64)
        xs = xs * delta + lower
    mod_ref = MEANS[mean](g)
    Z = (0.05 + 0.9 * torch.rand(int(np.prod(NPTS)), 2, generator=g, dtype=torch.float64)) if learn else None
    m = RefShapedGDRF(xs, ws, kind="rbf", K=K, n_points=NPTS, dtype=torch.float64, jitter=1e-6, lengthscale=0.2, Z=Z, learn_inducing=learn,
                      whiten=whiten, mean_function=mod_ref, world=WORLD if world else None, link_function=link, optimizer=opt, lr=lr)
    perturb_posterior(m, g)
    ls = [0.15, 0.3] if ard else 0.2
    if ard:
        m.params["log_lengthscale"] = torch.tensor(ls, dtype=torch.float64).log().requires_grad_(True)
    mod = copy.deepcopy(mod_ref).to(DEV)
    xs_d, ws_d = xs.to(DEV, dtype), torch.from_numpy(ws).to(DEV)
    model = SparseMultinomialGDRF(xs=xs_d, ws=ws_d, world=WORLD if world else [(0.0, 1.0)] * 2,
                                  kernel=RBF(input_dim=2, lengthscale=ls, variance=torch.tensor(25.0)), num_observation_categories=V,
                                  num_topic_categories=K, dirichlet_param=m.alpha, n_points=list(NPTS), fixed_inducing_points=not learn,
                                  inducing_points=m.Z, maxjitter=15, jitter=1e-6, device=DEV, dtype=dtype, whiten=whiten,
                                  mean_function=mod, link_function=link, seed=seed)
    eng = model._engine
    for name, p in m.params.items():
        eng.view(name).copy_(p.detach().reshape(eng.view(name).shape))
    sc = poutine.scale(scale=1.0 / m.N)
    objective = Trace_ELBO(num_particles=P) if renyi is None else RenyiELBO(alpha=renyi, num_particles=P)
    svi = SVI(model=sc(model.model), guide=sc(model.guide), optim=OPTIMIZER_DICT[opt]({"lr": lr}), loss=objective)
    eps = torch.randn(P, K, m.N, generator=g, dtype=torch.float64)
    return m, model, svi, eps, xs_d, ws_d, mod_ref


def oracle_loss(m, eps, renyi=None):
    if renyi is not None:
        return m.renyi_loss(eps, renyi)
    return sum(m.loss(eps[p]) for p in range(eps.shape[0])) / eps.shape[0]


def check_step(mean="trend_kn", dtype=torch.float64, renyi=None, **kw):
    m, model, svi, eps, xs, ws, mod_ref = setup(mean=mean, dtype=dtype, renyi=renyi, **kw)
    eng = model._engine
    loss = svi.step(xs=xs, ws=ws, subsample=False, eps=eps)
    m.force_jitter_level = eng.last_jitter_level
    ref = oracle_loss(m, eps, renyi)
    names, ps = list(m.params), list(m.params.values())
    mps = list(mod_ref.named_parameters())
    grads = torch.autograd.grad(ref, ps + [p for _, p in mps], allow_unused=True)
    grads = [torch.zeros_like(p) if gr is None else gr for gr, p in zip(grads, ps + [p for _, p in mps])]
    gmax = max(float(gr.abs().max()) for gr in grads)
    tl, tg, tm = (LOSS_TOL_VS_TORCH, 1e-7, 1e-8) if dtype == torch.float64 else (2e-5, 5e-3, 5e-3)
    assert abs(loss - float(ref)) <= tl * abs(float(ref)), (loss, float(ref))
    for name, gr in zip(names, grads):
        assert relerr(eng.view(name, eng.grads).cpu().numpy(), gr.numpy(), 1e-3 * gmax) < tg, name
    mean_grads = {}
    for (name, _), gr in zip(mps, grads[len(ps):]):
        got = eng.view("_mean_function." + name, eng.grads).cpu().double()
        assert got.shape == gr.shape
        assert relerr(got.numpy(), gr.numpy(), 1e-3 * gmax if dtype == torch.float32 else 1e-6 * gmax) < tm, name
        mean_grads[name] = (got, gr, gmax)
    return mean_grads


@pytest.mark.parametrize("mean", ["const", "trend_kn"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_mean_gradient_matches_autograd(mean, dtype):
    mg = check_step(mean=mean, dtype=dtype)
    got, ref, gmax = next(iter(mg.values()))
    assert float(ref.abs().max()) > 1e-4 * gmax                     # not a vacuous case


def test_shared_trend_has_zero_gradient_under_softmax_but_not_under_a_custom_link():
    got, ref, gmax = check_step(mean="trend_n")["w"]
    assert float(got.abs().max()) < 1e-8 * gmax                     # softmax(mu + c) = softmax(mu)
    got, ref, gmax = check_step(mean="trend_n", link=SIGMOID_LINK)["w"]
    assert float(ref.abs().max()) > 1e-4 * gmax


@pytest.mark.parametrize("case", ["unwhitened", "learn_inducing", "ard", "particles", "renyi", "world", "link"])
def test_mean_gradient_in_every_path(case):
    kw = dict(unwhitened=dict(whiten=False), learn_inducing=dict(learn=True), ard=dict(ard=True), particles=dict(P=3),
              renyi=dict(P=3, renyi=0.5), world=dict(world=True), link=dict(link=SIGMOID_LINK))[case]
    mg = check_step(mean="trend_kn", **kw)
    got, ref, gmax = mg["w"]
    assert float(ref.abs().max()) > 1e-4 * gmax


def test_non_unit_world_differentiates_both_mean_evaluations():
    """The guide's mean at scale(scale(xs)) and the model's at scale(xs) both reach the gradient: dropping either changes it."""
    m, model, svi, eps, xs, ws, mod_ref = setup(world=True)
    xs_m = m.scale(m.xs)
    xs_g = m.scale(xs_m)
    svi.step(xs=xs, ws=ws, subsample=False, eps=eps)
    m.force_jitter_level = model._engine.last_jitter_level
    ref = m.loss(eps[0])
    (gw,) = torch.autograd.grad(ref, [mod_ref.w])
    got = model._engine.view("_mean_function.w", model._engine.grads).cpu()
    assert relerr(got.numpy(), gw.numpy()) < 1e-8
    # with either evaluation held constant (the oracle's loss calls the guide's first, then the model's) the gradient moves by far more
    # than the tolerance above
    for held in (0, 1):
        calls = []

        def mf(x, held=held):
            calls.append(x)
            return mod_ref(x).detach() if len(calls) - 1 == held else mod_ref(x)
        m.mean_function = mf
        (g1,) = torch.autograd.grad(m.loss(eps[0]), [mod_ref.w])
        assert len(calls) == 2 and torch.allclose(calls[0], xs_g) and torch.allclose(calls[1], xs_m)
        assert float((g1 - gw).abs().max()) > 1e-5 * float(gw.abs().max())


@pytest.mark.parametrize("opt", ["adam", "adamw", "clippedadam"])
def test_five_steps_follow_torch_optimizers_on_the_module(opt):
    """SVI.step updates the module's parameters with the arithmetic, step count and learning rate of the model's own: the oracle
    with its per-parameter optimizers plus the matching torch optimizer on the reference module.  Fails when the mean stays put."""
    lr = 5e-2
    m, model, svi, eps0, xs, ws, mod_ref = setup(opt=opt, lr=lr)
    mod = model._mean_function
    w0 = mod.w.detach().clone()
    mopt = {"adam": lambda p: torch.optim.Adam([p], lr=lr), "adamw": lambda p: torch.optim.AdamW([p], lr=lr),
            "clippedadam": lambda p: _ClippedAdam(p, lr=lr)}[opt](mod_ref.w)
    g = torch.Generator().manual_seed(17)
    for step in range(5):
        eps = torch.randn(K, m.N, generator=g, dtype=torch.float64)
        loss = svi.step(xs=xs, ws=ws, subsample=False, eps=eps)
        m.force_jitter_level = model._engine.last_jitter_level
        mod_ref.w.grad = None
        loss_ref = m.step(eps)
        mopt.step()
        assert abs(loss - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref), (step, loss, loss_ref)
        assert mod.w.dtype == torch.float64 and mod.w.device == torch.device(DEV)
        assert relerr(mod.w.detach().cpu().numpy(), mod_ref.w.detach().numpy()) < 1e-7, step
    assert float((mod.w.detach() - w0).abs().max()) > 10 * lr * 0.1             # the mean did move
    st = svi.optim.get_state()["_mean_function.w"]
    assert st["step"] == 5 and st["exp_avg"].shape == mod.w.shape


@pytest.mark.parametrize("kind", ["lambda", "frozen"])
def test_plain_callables_and_frozen_modules_take_the_data_path(kind):
    """A lambda and a module without trainable parameters: no mean segment, and loss and grads bitwise those of passing the same
    values as data through Engine.loss_and_grads(mean=...)."""
    from gdrf_amd import poutine
    from gdrf_amd.infer import SVI, Trace_ELBO
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    from gdrf_amd.optim import Adam
    g = torch.Generator().manual_seed(5)
    trend = TrendKN(g).to(DEV)
    if kind == "frozen":
        trend.requires_grad_(False)
        fn = trend
    else:
        w = trend.w.detach()
        fn = lambda x: w[:, :-1] @ x.T + w[:, -1:]       # noqa: E731
    xs_np, ws_np, _ = synth_circles(15, 11, V, K, seed=3)
    xs, ws = torch.from_numpy(xs_np).to(DEV, torch.float64), torch.from_numpy(ws_np).to(DEV)
    model = SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2, kernel=RBF(input_dim=2, lengthscale=0.2, variance=torch.tensor(25.0)),
                                  num_observation_categories=V, num_topic_categories=K, dirichlet_param=0.01, n_points=list(NPTS),
                                  fixed_inducing_points=True, inducing_init="grid", maxjitter=15, jitter=1e-6, device=DEV, dtype=torch.float64,
                                  mean_function=fn)
    eng = model._engine
    assert eng.mean_count == 0 and eng.red_layout["mean"] == eng.red_layout["total_d"]
    eps = torch.randn(1, K, xs.shape[0], generator=g, dtype=torch.float64).to(DEV)
    eng.loss_and_grads(xs, ws.int(), eps, n_global=1.0 / (1.0 / xs.shape[0]), mean=fn(xs))     # SVI's 1 / scale
    loss0, grads0 = eng.read_out()["loss"], eng.grads.clone()
    sc = poutine.scale(scale=1.0 / xs.shape[0])
    svi = SVI(model=sc(model.model), guide=sc(model.guide), optim=Adam({"lr": 1e-2}), loss=Trace_ELBO())
    loss = svi.step(xs=xs, ws=ws, subsample=False, eps=eps)
    assert loss == loss0
    assert torch.equal(eng.grads, grads0)


def _dist_build():
    m, model, svi, _, xs, ws, _ = setup()
    return model, svi, xs, ws


def _save_w(model):
    return {"w": model._mean_function.w.detach().cpu()}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("via", ["torch_distributed", "c_abi_hook"])
def test_two_ranks_on_one_gpu_match_a_single_rank(tmp_path, via):
    """The mean segment rides in the step's single collective: two ranks on halves of the rows train the module like one rank."""
    port = 29800 + (os.getpid() % 2000) + (7 if via == "c_abi_hook" else 0)
    r0, r1 = run_two_ranks(_dist_build, via, port, tmp_path, save=_save_w)
    m, model, svi, _, xs, ws, _ = setup()
    w0 = model._mean_function.w.detach().cpu().clone()
    ref = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(3)]
    assert np.allclose(r0["losses"], ref, rtol=1e-10)
    assert torch.equal(r0["w"], r1["w"])
    w = model._mean_function.w.detach().cpu()
    assert float((w - w0).abs().max()) > 1e-3
    assert float((r0["w"] - w).abs().max()) < 1e-9


def test_checkpoint_restores_the_trained_mean(tmp_path):
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    m, model, svi, _, xs, ws, _ = setup()
    for _ in range(3):
        svi.step(xs=xs, ws=ws, subsample=False)
    snap = copy.deepcopy(model)
    assert "_mean_function.w" in snap.state_dict()
    torch.save({"model": snap}, tmp_path / "ckpt.pt")
    torch.serialization.add_safe_globals([ModelSnapshot])
    loaded = torch.load(tmp_path / "ckpt.pt", weights_only=True)["model"]
    fresh = TrendKN(torch.Generator().manual_seed(99)).to(DEV)
    restored = loaded.restore(mean_function=fresh)
    assert torch.equal(fresh.w.detach(), model._mean_function.w.detach())
    wp = model.word_probs(xs).cpu().numpy()
    assert relerr(restored.word_probs(xs).cpu().numpy(), wp) < 1e-12
    # a restore without the module rebuilds the predictive surface and leaves the mean entries aside
    assert relerr(loaded.restore().word_probs(xs).cpu().numpy(), wp) < 1e-12
