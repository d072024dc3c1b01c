"""The pyro.optim rules of gdrf/train_script.py:73-87 beyond the plain Adam family, with clip_args and per-parameter optim_args callables,
on the GPU (gdrf_optim_step): injected gradients against torch.optim with one optimizer per parameter tensor, determinism, SVI against
the oracle's gradients stepped by torch optimizers, the state lifecycle, train() and a failed Cholesky factorisation."""
import math

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import RefShapedGDRF, synth_circles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 6
LOSS_TOL_VS_TORCH = 1e-6          # as in tests/test_gpu_parity.py
MEAN = {"_mean_function.w": (3, 2), "_mean_function.b": (2,)}

TORCH = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "adamax": torch.optim.Adamax, "rmsprop": torch.optim.RMSprop,
         "adagrad": torch.optim.Adagrad, "adadelta": torch.optim.Adadelta, "asgd": torch.optim.ASGD, "rprop": torch.optim.Rprop}

CASES = [("adamax", {}), ("adamax", {"lr": 1e-2, "weight_decay": 0.1, "betas": (0.8, 0.99)}),
         ("rmsprop", {}), ("rmsprop", {"momentum": 0.9, "centered": True, "weight_decay": 0.1}), ("rmsprop", {"centered": True}),
         ("rmsprop", {"momentum": 0.5, "alpha": 0.9}),
         ("adagrad", {}), ("adagrad", {"lr_decay": 0.1, "initial_accumulator_value": 0.5, "weight_decay": 0.1}),
         ("adadelta", {}), ("adadelta", {"rho": 0.8, "weight_decay": 0.1, "lr": 0.5}),
         ("asgd", {}), ("asgd", {"t0": 2.0, "lambd": 1e-2, "alpha": 0.5, "weight_decay": 0.1}),
         ("rprop", {}), ("rprop", {"etas": (0.3, 1.5), "step_sizes": (1e-3, 0.05)}),
         ("adagradrmsprop", {}), ("adagradrmsprop", {"eta": 0.1, "t": 0.3})]


class _AdagradRMSProp:
    """pyro 1.8.0 AdagradRMSProp, restated: sum = g^2 at the first step, then (1 - t) sum + t g^2; p -= eta step^(-1/2 + delta) g / (1 + sqrt(sum))."""

    def __init__(self, params, eta=1.0, delta=1e-16, t=0.1):
        self.p, self.eta, self.delta, self.t = params[0], eta, delta, t
        self.state = {self.p: {"step": 0}}

    def step(self):
        st, g = self.state[self.p], self.p.grad
        st["step"] += 1
        st["sum"] = g * g if st["step"] == 1 else (1.0 - self.t) * st["sum"] + self.t * g * g
        with torch.no_grad():
            self.p -= self.eta * st["step"] ** (-0.5 + self.delta) * g / (1.0 + st["sum"].sqrt())


class f64_scalars:
    """torch >= 2 keeps ASGD's eta and mu (and step counts) as tensors of the default dtype, float32 unless it is float64; torch 1.9.1,
    the version the reference pins, kept Python floats.  Step the reference with float64 scalars."""

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


def torch_opt(name, p, args):
    if name == "adagradrmsprop":
        return _AdagradRMSProp([p], **args)
    return TORCH[name]([p], foreach=False, **args)


def make_engine(dtype, seed=0, mean=False):
    from gdrf_amd.engine import Engine
    eng = Engine(8, 6, 3, 7, 2, dtype=dtype, device=DEV, process_group=None, mean_params=MEAN if mean else None)
    g = torch.Generator().manual_seed(seed)
    eng.params.copy_(torch.randn(eng.params.shape, generator=g, dtype=torch.float64))
    return eng


def gradients(eng, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(eng.grads.shape, generator=g, dtype=torch.float64).to(eng.dtype) for _ in range(STEPS)]


def clip_ref(p, clip):
    if "clip_norm" in clip:
        torch.nn.utils.clip_grad_norm_([p], clip["clip_norm"])
    if "clip_value" in clip:
        torch.nn.utils.clip_grad_value_([p], clip["clip_value"])


def run_pair(name, args, dtype, clip_args=None, mean=False, grads_fn=None):
    """STEPS steps of gdrf_amd.optim on injected gradients and of torch (CPU, float64, one optimizer per parameter tensor)."""
    from gdrf_amd.optim import OPTIMIZER_DICT, param_store_name
    eng = make_engine(dtype, mean=mean)
    p0 = eng.params.clone()
    o = OPTIMIZER_DICT[name](args, clip_args)
    o._bind(eng)
    ref = {n: torch.nn.Parameter(v.detach().cpu().double().clone()) for n, v in eng.named_views().items()}
    opts = {n: torch_opt(name, p, o.args_for(n)) for n, p in ref.items()}
    clips = {n: (clip_args(param_store_name(n), param_store_name(n)) if callable(clip_args) else (clip_args or {})) for n in ref}
    G = gradients(eng) if grads_fn is None else grads_fn(eng)
    for step in range(STEPS):
        eng.grads.copy_(G[step])
        o._step()
        for n, p in ref.items():
            p.grad = eng.view(n, eng.grads).detach().cpu().double().clone()
            clip_ref(p, clips[n])
            with f64_scalars():
                opts[n].step()
    torch.cuda.synchronize()
    return eng, p0, o, ref, opts


def check_pair(eng, p0, o, ref, opts, dtype):
    st = o.get_state()
    for n, p in ref.items():
        got = eng.view(n).cpu().double()
        scale = float(p.detach().abs().max())
        tol = 1e-12 * scale if dtype == torch.float64 else 1e-5 * scale
        assert float((got - p.detach()).abs().max()) <= tol, (n, float((got - p.detach()).abs().max()), scale)
        tst = opts[n].state[p]
        assert int(st[n]["step"]) == int(tst["step"]) == STEPS
        keys = [k for k in tst if k not in ("step", "eta", "mu")]
        assert keys and set(keys) == set(st[n]) - {"step", "lr", "eta", "mu"}, (n, keys, list(st[n]))
        for k in keys:
            want = tst[k].double()
            sc = max(float(want.abs().max()), 1e-300)
            err = float((st[n][k].cpu().double() - want).abs().max())
            assert err <= (1e-12 if dtype == torch.float64 else 1e-5) * max(sc, 1e-3), (n, k, err, sc)
        for k in ("eta", "mu"):
            if k in tst:
                assert math.isclose(float(st[n][k]), float(tst[k]), rel_tol=1e-12), (n, k)
    # elements outside every learnt parameter tensor (log_scale_mixture under RBF, the inducing-input block) are untouched
    mask = torch.ones(eng.params.numel(), dtype=torch.bool)
    for off, ln in eng.segments().values():
        mask[off:off + ln] = False
    assert mask.any() and torch.equal(eng.params.cpu()[mask], p0.cpu()[mask])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,args", CASES, ids=[f"{n}-{i}" for i, (n, _) in enumerate(CASES)])
def test_rules_follow_torch_with_injected_gradients(name, args, dtype):
    eng, p0, o, ref, opts = run_pair(name, args, dtype)
    assert float((eng.params - p0).abs().max()) > 0
    check_pair(eng, p0, o, ref, opts, dtype)


def _clippable_grads(eng):
    """Gradients whose u_scale_tril block is far longer than 3 and whose scalar blocks are shorter: clip_norm = 3 clips one, not the others."""
    G = [torch.randn(eng.grads.shape, generator=torch.Generator().manual_seed(11 + s), dtype=torch.float64).to(eng.dtype) for s in range(STEPS)]
    for g in G:
        g[eng.layout["log_variance"]] = 0.5
        g[eng.layout["log_noise"]] = -0.25
    return G


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,args,clip", [
    ("adam", {"lr": 1e-2}, {"clip_norm": 3.0}),
    ("adamw", {"lr": 1e-2}, {"clip_norm": 3.0, "clip_value": 0.2}),
    ("rmsprop", {"momentum": 0.9, "centered": True}, {"clip_norm": 3.0}),
    ("adagrad", {}, {"clip_value": 0.3}),
    ("rprop", {}, {"clip_norm": 3.0}),
    ("adamax", {}, lambda m, p: {"clip_norm": 3.0} if p == "u_scale_tril" else ({"clip_value": 0.1} if p == "u_loc" else {})),
])
def test_clip_args_follow_clip_grad_then_the_torch_step(name, args, clip, dtype):
    eng, p0, o, ref, opts = run_pair(name, args, dtype, clip_args=clip, grads_fn=_clippable_grads)
    g = _clippable_grads(eng)[0].cpu().double()
    if not callable(clip) and "clip_norm" in clip:
        norms = {n: float(eng.view(n, g).norm()) for n in eng.param_names}
        assert norms["u_scale_tril_unc"] > 3.0 and norms["log_variance"] < 3.0        # one segment clipped, another not
    check_pair(eng, p0, o, ref, opts, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_adam_with_a_callable_giving_u_loc_its_own_lr(dtype):
    lrs = {"u_loc": 0.2, "_mean_function.w": 0.05}
    seen = []

    def args(module_name, param_name):
        seen.append(param_name)
        return {"lr": lrs.get(param_name, 1e-2)}
    eng, p0, o, ref, opts = run_pair("adam", args, dtype, mean=True)
    assert "u_loc" in seen and "_kernel.lengthscale" in seen and "_mean_function.w" in seen and len(seen) == len(set(seen))
    assert o.args_for("u_loc")["lr"] == 0.2 and o.args_for("phi_unc")["lr"] == 1e-2
    check_pair(eng, p0, o, ref, opts, dtype)


def test_two_engines_end_bitwise_equal():
    from gdrf_amd.optim import RMSprop
    outs = []
    for _ in range(2):
        eng = make_engine(torch.float32)
        o = RMSprop({"momentum": 0.9, "centered": True}, {"clip_norm": 3.0})
        o._bind(eng)
        for g in _clippable_grads(eng):
            eng.grads.copy_(g)
            o._step()
        torch.cuda.synchronize()
        outs.append([eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.opt_extra.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- SVI level (fp64: DESIGN.md, fp32 trajectories are not comparable) -----------------------------------------------------------
K, V, NPTS = 4, 20, (6, 4)


def svi_setup(opt, mean_function=None, mod_ref=None):
    from gdrf_amd import poutine
    from gdrf_amd.infer import SVI, Trace_ELBO
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    xs, ws, _ = synth_circles(18, 12, V, K, seed=3)
    xs_t = torch.from_numpy(xs).double()
    g = torch.Generator().manual_seed(103)
    m = RefShapedGDRF(xs_t, ws, kind="rbf", K=K, n_points=NPTS, dtype=torch.float64, jitter=1e-6, lengthscale=0.2, mean_function=mod_ref)
    with torch.no_grad():
        m.params["u_loc"].add_(0.3 * torch.randn(m.params["u_loc"].shape, generator=g, dtype=torch.float64))
        m.params["phi_unc"].add_(0.5 * torch.randn(m.params["phi_unc"].shape, generator=g, dtype=torch.float64))
    xs_d, ws_d = xs_t.to(DEV), torch.from_numpy(ws).to(DEV)
    model = SparseMultinomialGDRF(xs=xs_d, ws=ws_d, world=[(0.0, 1.0)] * 2, kernel=RBF(input_dim=2, lengthscale=0.2, variance=torch.tensor(25.0)),
                                  num_observation_categories=V, num_topic_categories=K, dirichlet_param=m.alpha, n_points=list(NPTS),
                                  fixed_inducing_points=True, inducing_points=m.Z, maxjitter=15, jitter=1e-6, device=DEV,
                                  dtype=torch.float64, mean_function=mean_function, seed=3)
    for name, p in m.params.items():
        model._engine.view(name).copy_(p.detach())
    sc = poutine.scale(scale=1.0 / m.N)
    svi = SVI(model=sc(model.model), guide=sc(model.guide), optim=opt, loss=Trace_ELBO(num_particles=1))
    return m, model, svi, xs_d, ws_d


@pytest.mark.parametrize("name,args", [("rmsprop", {"lr": 1e-2, "momentum": 0.5, "centered": True}), ("adagrad", {"lr": 5e-2}),
                                       ("rprop", {"lr": 1e-2})])
def test_svi_five_steps_fp64_follow_torch_on_the_oracle(name, args):
    from gdrf_amd.optim import OPTIMIZER_DICT
    m, model, svi, xs, ws = svi_setup(OPTIMIZER_DICT[name](args))
    opts = {n: torch_opt(name, p, dict(args)) for n, p in m.params.items()}
    g = torch.Generator().manual_seed(5)
    for step in range(5):
        eps = torch.randn(K, m.N, generator=g, dtype=torch.float64)
        loss = svi.step(xs=xs, ws=ws, subsample=False, eps=eps)
        m.force_jitter_level = model._engine.last_jitter_level
        loss_ref, _ = m.loss_and_grads(eps)
        for o in opts.values():
            o.step()
        assert abs(loss - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref), (step, loss, loss_ref)
    eng = model._engine
    for n in eng.param_names:
        a, b = eng.view(n).cpu().numpy(), m.params[n].detach().numpy()
        assert np.abs(a - b).max() <= 1e-8 * (np.abs(b).max() + 1e-300), n


# ---- state lifecycle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", [("rmsprop", {"momentum": 0.9, "centered": True}), ("asgd", {"t0": 2.0, "lambd": 1e-2}),
                                       ("rprop", {}), ("clippedadam", {"lrd": 0.9})])
def test_state_round_trip_mid_run_continues_bitwise(name, args):
    from gdrf_amd.optim import OPTIMIZER_DICT
    clip = {"clip_norm": 3.0}
    ea = make_engine(torch.float32)
    oa = OPTIMIZER_DICT[name](args, clip)
    oa._bind(ea)
    G = _clippable_grads(ea)
    for s in range(3):
        ea.grads.copy_(G[s]); oa._step()
    state = oa.get_state()
    eb = make_engine(torch.float32, seed=9)                 # different parameters: the state alone is restored
    eb.params.copy_(ea.params)
    ob = OPTIMIZER_DICT[name](args, clip)
    ob.set_state(state)
    ob._bind(eb)
    for s in range(3, STEPS):
        ea.grads.copy_(G[s]); oa._step()
        eb.grads.copy_(G[s]); ob._step()
    torch.cuda.synchronize()
    assert torch.equal(ea.params, eb.params)
    sa, sb = oa.get_state(), ob.get_state()
    for n in sa:
        for k in sa[n]:
            assert torch.equal(torch.as_tensor(sa[n][k]), torch.as_tensor(sb[n][k])), (n, k)


def test_state_is_carried_across_engine_growth():
    """n rows, then 2n rows: the model grows its engine and every state vector (the third one included) comes along."""
    from gdrf_amd.optim import RMSprop
    xs, ws, _ = synth_circles(10, 6, V, K, seed=4)
    xs, ws = torch.from_numpy(xs).double().to(DEV), torch.from_numpy(ws).to(DEV)
    n = xs.shape[0] // 2

    def run(split):
        from gdrf_amd import poutine
        from gdrf_amd.infer import SVI, Trace_ELBO
        from gdrf_amd.kernels import RBF
        from gdrf_amd.models import SparseMultinomialGDRF
        model = SparseMultinomialGDRF(xs=xs[:n] if split else xs, ws=ws[:n] if split else ws, world=[(0.0, 1.0)] * 2,
                                      kernel=RBF(input_dim=2, lengthscale=0.2, variance=torch.tensor(25.0)), num_observation_categories=V,
                                      num_topic_categories=K, dirichlet_param=0.01, n_points=list(NPTS), fixed_inducing_points=True,
                                      inducing_init="grid", maxjitter=15, jitter=1e-6, device=DEV, dtype=torch.float64, seed=3)
        opt = RMSprop({"lr": 1e-2, "momentum": 0.9, "centered": True})
        svi = SVI(model=poutine.scale(scale=1.0 / n)(model.model), guide=poutine.scale(scale=1.0 / n)(model.guide), optim=opt,
                  loss=Trace_ELBO(num_particles=1))
        g = torch.Generator().manual_seed(6)
        caps = []
        for step in range(4):
            rows = n if step < 2 else 2 * n
            eps = torch.randn(K, rows, generator=g, dtype=torch.float64)
            svi.step(xs=xs[:rows], ws=ws[:rows], eps=eps)
            caps.append(model._engine.n_cap)
        return model._engine, opt, caps

    ea, oa, caps = run(True)
    eb, ob, capsb = run(False)
    assert caps == [n, n, 2 * n, 2 * n] and capsb == [2 * n] * 4 and ea.opt_extra is not None
    for a, b in [(ea.params, eb.params), (ea.exp_avg, eb.exp_avg), (ea.exp_avg_sq, eb.exp_avg_sq), (ea.opt_extra, eb.opt_extra)]:
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())          # the workspaces' sizes differ, the arithmetic not


class _Trend(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([[0.3, -0.2, 0.1]] * K, dtype=torch.float64))

    def forward(self, x):
        x = x.to(self.w.dtype)
        return self.w[:, :-1] @ x.T + self.w[:, -1:]


def test_mean_function_module_trains_under_rmsprop_like_torch():
    import copy
    from gdrf_amd.optim import RMSprop
    mod_ref = _Trend()
    mod = copy.deepcopy(mod_ref).to(DEV)
    lr = 1e-2
    m, model, svi, xs, ws = svi_setup(RMSprop({"lr": lr}), mean_function=mod, mod_ref=mod_ref)
    opts = {n: torch.optim.RMSprop([p], lr=lr, foreach=False) for n, p in m.params.items()}
    mopt = torch.optim.RMSprop([mod_ref.w], lr=lr, foreach=False)
    w0 = mod.w.detach().clone()
    g = torch.Generator().manual_seed(8)
    for step in range(5):
        eps = torch.randn(K, m.N, generator=g, dtype=torch.float64)
        loss = svi.step(xs=xs, ws=ws, subsample=False, eps=eps)
        m.force_jitter_level = model._engine.last_jitter_level
        mod_ref.w.grad = None
        loss_ref, _ = m.loss_and_grads(eps)
        for o in opts.values():
            o.step()
        mopt.step()
        assert abs(loss - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref), (step, loss, loss_ref)
        # RMSprop's first steps are about lr sign(g) / sqrt(1 - alpha): the tiny gradient differences of the fused path reach the
        # parameters almost undivided, hence 1e-6 here instead of the 1e-7 of the Adam family (tests/test_gpu_mean_params.py)
        a, b = mod.w.detach().cpu().numpy(), mod_ref.w.detach().numpy()
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), step
    assert float((mod.w.detach() - w0).abs().max()) > lr
    st = svi.optim.get_state()["_mean_function.w"]
    assert st["step"] == 5 and set(st) == {"step", "square_avg", "lr"}


def test_train_with_adamax_returns_a_finite_history():
    from gdrf_amd.train import train
    xs, ws, _ = synth_circles(16, 10, 12, 3, seed=2)
    out = train(xs=xs, ws=ws, dimensions=2, epochs=20, num_topics=3, num_inducing_points=[4, 3], inducing_initialization_method="grid",
                kernel_lengthscale=0.2, optimizer_type="adamax", optimizer_lr=0.01, jitter=1e-6)
    h = out["history"]
    assert h.shape[0] == 20 and np.isfinite(h).all()
    assert type(out["optimizer"]).__name__ == "Adamax" and out["model"]._engine.opt_step == 20


@pytest.mark.parametrize("name,clip", [("rmsprop", {"clip_norm": 3.0}), ("asgd", None), ("adagradrmsprop", {"clip_value": 0.1})])
def test_failed_cholesky_leaves_parameters_and_state_untouched(name, clip):
    """A negative jitter makes the first pivot of K_uu + jitter I negative: the factorisation fails deterministically, the device flag
    stays set, and the next update must change nothing."""
    from gdrf_amd.engine import Engine
    from gdrf_amd.optim import OPTIMIZER_DICT
    eng = Engine(8, 6, 3, 7, 2, dtype=torch.float64, device=DEV, process_group=None, jitter=-50.0, maxjitter=1)
    eng.params.copy_(torch.randn(eng.params.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64))
    eng.view("log_variance").fill_(0.0)
    eng.set_inducing_points(torch.rand(6, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64))
    o = OPTIMIZER_DICT[name]({}, clip)
    o._bind(eng)
    G = _clippable_grads(eng)
    for s in range(2):
        eng.grads.copy_(G[s]); o._step()
    with pytest.raises(RuntimeError, match="max jitter"):
        eng.factorize(force_level=0)
    before = [eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone()]
    eng.grads.copy_(G[2]); o._step()
    torch.cuda.synchronize()
    for a, b in zip(before, [eng.params, eng.exp_avg, eng.exp_avg_sq]):
        assert torch.equal(a, b)
