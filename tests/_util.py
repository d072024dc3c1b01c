"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import os
import sys

import numpy as np
import torch

from oracle.gdrf_oracle import RefShapedGDRF, fused_elbo_and_grads, jitter_total, synth_circles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_TOL_VS_TORCH = 1e-6          # torch's float32 lgamma of the int32 counts (tests/test_gpu_parity.py)
NAME_MAP = dict(log_lengthscale="log_lengthscale", log_variance="log_variance", log_noise="log_noise",
                u_loc="u_loc", phi_unc="phi_unc", u_scale_tril_unc="u_scale_tril_unc")


def perturb_posterior(m, g, s_perturb=0.1, trained_scale=None):
    """Move the oracle's variational parameters, phi and the noise off their initial values with draws from ``g``."""
    dtype, p = m.dtype, m.params
    with torch.no_grad():
        p["u_loc"].add_(0.3 * torch.randn(p["u_loc"].shape, generator=g, dtype=torch.float64).to(dtype))
        if trained_scale is not None:
            # a posterior that has contracted, as after training: S_k = trained_scale I + small lower-triangular noise (the
            # initial S_k = L_uu of sparse_gdrf.py:100-110 makes tt = |S^T w|^2 - hence mu = loc + v eps - as large as cond(K_uu))
            u = s_perturb * torch.randn(p["u_scale_tril_unc"].shape, generator=g, dtype=torch.float64).tril(-1)
            u = u + torch.diag_embed(torch.full(p["u_loc"].shape, float(np.log(trained_scale)), dtype=torch.float64))
            p["u_scale_tril_unc"].copy_(u.to(dtype))
        else:
            p["u_scale_tril_unc"].add_(s_perturb * torch.randn(p["u_scale_tril_unc"].shape, generator=g, dtype=torch.float64).tril().to(dtype))
        p["phi_unc"].add_(0.5 * torch.randn(p["phi_unc"].shape, generator=g, dtype=torch.float64).to(dtype))
        p["log_noise"].add_(0.2)


def make_oracle(kind="rbf", W=16, H=9, V=20, K=4, n_points=(4, 3), dtype=torch.float64, seed=1, jitter=1e-6,
                perturb=True, one_d=False, optimizer="adam", lr=1e-3, force_jitter_level=None, lengthscale=0.1,
                learn_inducing=False, random_inducing=False, scale_mixture=1.0, whiten=True, mean_function=None, s_perturb=0.1, trained_scale=None):
    xs, ws, _ = synth_circles(W, H, V, K, seed=seed, one_d=one_d)
    g = torch.Generator().manual_seed(seed + 100)
    Z = None
    if random_inducing:          # interior points: grid points on the world's boundary have a vanishing sigmoid Jacobian
        M = int(np.prod(n_points)) if not one_d else int(n_points[0])
        Z = 0.05 + 0.9 * torch.rand(M, 1 if one_d else 2, generator=g, dtype=torch.float64)
    m = RefShapedGDRF(xs, ws, kind=kind, K=K, n_points=n_points, dtype=dtype, jitter=jitter, optimizer=optimizer, lr=lr,
                      force_jitter_level=force_jitter_level, lengthscale=lengthscale, Z=Z, learn_inducing=learn_inducing,
                      scale_mixture=scale_mixture, whiten=whiten, mean_function=mean_function)
    if perturb:
        perturb_posterior(m, g, s_perturb, trained_scale)
    eps = torch.randn(K, m.N, generator=g, dtype=torch.float64).to(dtype)
    return m, eps


NPTS = {1: (8,), 2: (4, 3), 3: (3, 3, 2)}      # inducing grids of the variant oracles, by input dimension


def grid_inputs(D, seed=1, W=16, H=9, V=20, K=4, g=None):
    """(xs (N, D) float64 tensor, ws) of the synthetic grid; a third axis is uniform noise drawn from ``g`` (default: a generator of its
    own, seeded with ``seed``)."""
    xs, ws, _ = synth_circles(W, H, V, K, seed=seed, one_d=(D == 1))
    xs = torch.from_numpy(xs).double()
    if D == 3:
        g = torch.Generator().manual_seed(seed) if g is None else g
        xs = torch.cat([xs, torch.rand(xs.shape[0], 1, generator=g, dtype=torch.float64)], 1)
    return xs, ws


def variant_oracle(D, finish, learn=False, whiten=True, dtype=torch.float64, seed=1, W=16, H=9, V=20, K=4, shared_generator=False, **kw):
    """(oracle, eps) for the ARD / Periodic / Product tests: RefShapedGDRF(**kw) on grid_inputs with NPTS[D] inducing points (random interior
    ones when they are learnt), ``finish(m)`` substituting the variant's kernel parameters, then the perturbed posterior.  One generator
    (seed + 100) draws Z, the perturbation and eps in that order - and, with ``shared_generator``, the third input axis before them."""
    g = torch.Generator().manual_seed(seed + 100)
    xs, ws = grid_inputs(D, seed, W, H, V, K, g=g if shared_generator else None)
    Z = (0.05 + 0.9 * torch.rand(int(np.prod(NPTS[D])), D, generator=g, dtype=torch.float64)) if learn else None
    m = RefShapedGDRF(xs, ws, K=K, n_points=NPTS[D], dtype=dtype, jitter=1e-6, Z=Z, learn_inducing=learn, whiten=whiten, **kw)
    finish(m)
    perturb_posterior(m, g)
    eps = torch.randn(K, m.N, generator=g, dtype=torch.float64).to(dtype)
    return m, eps


def engine_for(m, dtype=None, n_cap=None, **kw):
    """gdrf_amd.Engine holding exactly the oracle's parameters, inducing points and Dirichlet prior; the kernel kind, ARD, the period count
    and the factor table follow the oracle's parameters unless ``kw`` says otherwise (ard=False: the isotropic twin, which takes the
    first lengthscale)."""
    from gdrf_amd.engine import Engine
    p = m.params
    if m.kind == "product":
        kw["product"] = [dict(name=pre.rstrip("."), kind=kind, active_dims=dims, lengthscales=p[pre + "log_lengthscale"].numel(),
                              periods=p[pre + "log_period"].numel() if kind == "periodic" else 0) for pre, kind, dims in m.factor_spec]
    else:
        kw.setdefault("ard", p["log_lengthscale"].dim() == 1)
    if "log_period" in p:
        kw["period_count"] = p["log_period"].numel()
    eng = Engine(n_cap or m.N, m.M, m.K, m.V, m.D, dtype=dtype or m.dtype, kernel=m.kind, jitter=m.jitter, maxjitter=m.maxjitter,
                 process_group=None, learn_inducing=m.learn_inducing, whiten=m.whiten, **kw)
    eng.set_inducing_points(m.Z)
    eng.set_dirichlet(m.alpha)
    load_params(eng, m)
    return eng


def engine_from_oracle(m, dtype=None, device="cuda:0", n_cap=None, **kw):
    return engine_for(m, dtype=dtype, n_cap=n_cap, device=device, **kw)


def load_params(eng, m):
    for name in eng.param_names:
        v, p = eng.view(name), m.params[name].detach().to(eng.dtype)
        v.copy_(p.reshape(v.shape) if p.numel() == v.numel() else p.flatten()[0])


def dev(t, eng, dtype=None):
    return torch.as_tensor(t).to(device=eng.device, dtype=dtype or eng.dtype).contiguous()


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def check_grads(eng, grads_ref, tg=1e-7):
    gv = eng.named_views(eng.grads)
    assert set(gv) == set(grads_ref), (set(gv), set(grads_ref))
    for name, g in gv.items():
        assert tuple(g.shape) == tuple(grads_ref[name].shape), name
        assert relerr(g.cpu().numpy(), grads_ref[name].numpy()) < tg, (name, relerr(g.cpu().numpy(), grads_ref[name].numpy()))


def check_loss_and_grads(eng, m, eps, tg=1e-7, tl=LOSS_TOL_VS_TORCH, **kw):
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    eng.loss_and_grads(xs, ws, dev(eps, eng), **kw)
    out = eng.read_out()
    m.force_jitter_level = eng.last_jitter_level
    loss_ref, grads_ref = m.loss_and_grads(eps)
    assert abs(out["loss"] - loss_ref) <= tl * abs(loss_ref), (out["loss"], loss_ref)
    check_grads(eng, grads_ref, tg)
    return grads_ref


def save_params(model):
    return {"params": model._engine.params.cpu()}


def _dist_worker(rank, world, port, tmp, build, via, save):
    """One of two ranks on halves of the rows, both on the box's single GPU: three steps of ``build()`` = (model, svi, ..., xs, ws).
    ``via``: "torch_distributed" (the engine's own all-reduce) or "c_abi_hook" (the collective registered behind the C ABI -
    gdrf_set_allreduce / gdrf_payload_allreduce -, what a non-Python host would do with ncclAllReduce on its RCCL communicator)."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, svi, *_, xs, ws = build()
    N = len(xs)
    lo, hi = rank * N // world, (rank + 1) * N // world
    svi.row_offset = lo
    if via == "c_abi_hook":
        eng = model._engine_for(hi - lo)
        eng.pg = None

        def allreduce(buf, count, is_double, stream):
            assert buf == eng.red_T.data_ptr() and count == eng.red_T.numel() and is_double == (eng.dtype == torch.float64)
            dist.all_reduce(eng.red_T)
            return 0
        eng.set_allreduce(allreduce)
    losses = [svi.step(xs=xs[lo:hi], ws=ws[lo:hi], subsample=False) for _ in range(3)]
    torch.save(dict(save(model), losses=losses), os.path.join(tmp, f"r{rank}.pt"))
    dist.destroy_process_group()


def run_two_ranks(build, via, port, tmp_path, save=save_params):
    """Spawn the two ranks (``build`` and ``save`` are module-level functions: they travel by name) and return what each saved:
    {"losses": its three losses, **save(model)}."""
    import torch.multiprocessing as mp
    mp.spawn(_dist_worker, args=(2, port, str(tmp_path), build, via, save), nprocs=2, join=True)
    return [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in (0, 1)]
