"""GPU tests of the joint posterior at new inputs (gdrf_predict_cov, gdrf_sample_joint; csrc/predict_cov.h) against a float64 torch
restatement of its definition, written here with oracle.gdrf_oracle's kernel_matrix and jittercholesky for the pieces those cover:

    L L^T = K_uu + j_uu I;  W = K_*m L^-T;  loc_k = W u_k;  R = K_** - W W^T;  C_k = R + (W S_k)(W S_k)^T
    f[s,k,:] = W (u_k + S_k xi[s,k,:]) + G zeta[s,k,:] + mean[k,:],  G = cholesky(R + j I)
    (whiten=False: u_k, S_k are L^-1 u_k, L^-1 S_k)

Neither pyro nor the reference's own forward(full_cov=True) can be run (quirk Q10), so this restatement is the yardstick.  Bounds, relative
to the largest magnitude of the compared array: 1e-7 in float64 contexts (as the Periodic and Product parity tests pin them), 1e-4 in
float32 ones.  A float32 context is compared with the restatement at the same float32-valued parameters, rows and inducing inputs, and
both sides use the jitter levels the engine reports.  ARD, Periodic and Product kernels are restated as the isotropic RBF kernel_matrix on
the scaled / embedded coordinates (|e(x) - e(z)|^2 = 4 sin^2(pi (x - z) / p) / ls^2 for the pair (cos, sin)(2 pi x / p) / ls).

Largest figures seen on an MI355X are recorded in DESIGN.md section 19."""
import copy
import io
import math

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import jittercholesky, kernel_matrix
from tests._util import relerr

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-7, torch.float32: 1e-4}
JIT = {torch.float64: 1e-6, torch.float32: 1e-4}
DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
# every edge of the product kernel's tiling: the 16-row instruction tile, a wave's 32 x 32 quarter, the workgroup's 64 x 64 tile, two tiles
NS_COV = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
V = 3


def rnd(t, dtype):
    """float64 values that the context's element type represents exactly"""
    return t.to(dtype).double()


def grid_points(grid, M, span=1.0):
    """the first M points, last axis fastest, of the grid of `grid` points per axis on [0, span]^D"""
    axes = [torch.linspace(0.0, span, g, dtype=torch.float64) for g in grid]
    return torch.stack([a.flatten() for a in torch.meshgrid(*axes, indexing="ij")], -1).reshape(-1, len(grid))[:M]


class Case:
    """One engine and the float64 numbers it was loaded with.  kernel: "rbf", "matern52", "ard", "periodic" (D = 1) or "product"
    (RBF on axis 0 times Periodic on axis 1).  D: 2 unless given ("rbf", "matern52" and "ard" take up to GDRF_DMAX = 4).  grid: the
    inducing points are the first M points of that grid on [0, span]^D, and the rows are drawn from the same cube.  pure: the all-fp32
    context (dtype float32, the solves in float32 too).  engine=False: the numbers alone, no device."""

    def __init__(self, kernel, M, K, dtype, whiten=True, n_cap=129, seed=0, jitter=None, maxjitter=15, Z=None, ls=0.3, D=None, grid=None,
                 span=1.0, pure=False, engine=True):
        g = torch.Generator().manual_seed(10 * M + K + seed)
        self.kernel, self.M, self.K, self.dtype, self.whiten, self.pure, self.span = kernel, M, K, dtype, whiten, pure, span
        self.D = D = (1 if kernel == "periodic" else 2) if D is None else D
        self.grid = grid
        if grid is not None:
            assert Z is None and len(grid) == D and int(np.prod(grid)) >= M
            Z = grid_points(grid, M, span)
        self.Z = rnd(torch.rand(M, D, generator=g, dtype=torch.float64) if Z is None else torch.as_tensor(Z, dtype=torch.float64), dtype)
        self.u = rnd(0.5 * torch.randn(K, M, generator=g, dtype=torch.float64), dtype)
        s_unc = 0.1 * torch.randn(K, M, M, generator=g, dtype=torch.float64).tril(-1)
        s_unc = rnd(s_unc + torch.diag_embed(torch.full((K, M), math.log(0.3), dtype=torch.float64)), dtype)
        self.S = s_unc.tril(-1) + torch.diag_embed(s_unc.diagonal(dim1=1, dim2=2).exp())
        lg = lambda v: rnd(torch.as_tensor(v, dtype=torch.float64).log(), dtype)
        kw, self.hyp = {}, {}
        if kernel in ("rbf", "matern52"):
            self.hyp = dict(log_lengthscale=lg(ls), log_variance=lg(25.0))
        elif kernel == "ard":
            kw = dict(ard=True)
            self.hyp = dict(log_lengthscale=lg([0.25, 0.4] if D == 2 else [ls * (1 + 0.15 * d) for d in range(D)]), log_variance=lg(25.0))
        elif kernel == "periodic":
            kw = dict(period_count=1)
            self.hyp = dict(log_lengthscale=lg(0.8), log_variance=lg(4.0), log_period=lg(0.45))
        else:
            kw = dict(product=[dict(name="kern0", kind="rbf", active_dims=[0], lengthscales=1, periods=0),
                               dict(name="kern1", kind="periodic", active_dims=[1], lengthscales=1, periods=1)])
            self.hyp = {"kern0.log_variance": lg(2.0), "kern0.log_lengthscale": lg(0.4), "kern1.log_variance": lg(3.0),
                        "kern1.log_lengthscale": lg(0.8), "kern1.log_period": lg(0.45)}
        self.s_unc = s_unc
        self.jitter = JIT[dtype] if jitter is None else jitter
        if not engine:
            return
        from gdrf_amd.engine import Engine
        name = {"ard": "rbf"}.get(kernel, kernel)
        self.eng = eng = Engine(n_cap, M, K, V, D, dtype=dtype, kernel=name, jitter=self.jitter, maxjitter=maxjitter, process_group=None,
                                whiten=whiten, pure_fp32=pure, **kw)
        eng.set_inducing_points(self.Z)
        eng.view("u_loc").copy_(self.u)
        eng.view("u_scale_tril_unc").copy_(s_unc)
        for k, v in self.hyp.items():
            eng.view(k).copy_(v)

    def rows(self, n, seed=1, near=True):
        """n rows of the cube.  Grid cases with near: row 0 sits next to the LAST inducing point, where the last column of W - alone in
        its 32-column block when M = 32 b + 1 - carries most of the prior variance"""
        g = torch.Generator().manual_seed(n + seed)
        X = self.span * torch.rand(n, self.D, generator=g, dtype=torch.float64)
        if self.grid is not None and near:
            X[0] = self.Z[-1] * (1 - 1 / 64)
        return rnd(X, self.dtype)

    def dev(self, t):
        return torch.as_tensor(t).to(device=self.eng.device, dtype=self.dtype).contiguous()

    def kfun(self, X, Y):
        h = {k: v.exp() for k, v in self.hyp.items()}
        one = torch.tensor(1.0, dtype=torch.float64)
        if self.kernel in ("rbf", "matern52"):
            return kernel_matrix(self.kernel, X, Y, h["log_lengthscale"], h["log_variance"])
        if self.kernel == "ard":
            return kernel_matrix("rbf", X / h["log_lengthscale"], Y / h["log_lengthscale"], one, h["log_variance"])
        if self.kernel == "periodic":
            t, il = 2 * math.pi / h["log_period"], 1 / h["log_lengthscale"]
            e = lambda A: torch.cat([torch.cos(t * A), torch.sin(t * A)], 1) * il
            return kernel_matrix("rbf", e(X), e(Y), one, h["log_variance"])
        t, il = 2 * math.pi / h["kern1.log_period"], 1 / h["kern1.log_lengthscale"]
        e = lambda A: torch.cat([A[:, :1] / h["kern0.log_lengthscale"], torch.cos(t * A[:, 1:]) * il, torch.sin(t * A[:, 1:]) * il], 1)
        return kernel_matrix("rbf", e(X), e(Y), one, h["kern0.log_variance"] * h["kern1.log_variance"])

    def restate(self, X):
        """loc (K, n), R (n, n), C (K, n, n), W (n, M), and the u, S the predictive uses; at the engine's K_uu jitter level"""
        L, _ = jittercholesky(self.kfun(self.Z, self.Z), self.M, self.eng.jitter, self.eng.maxjitter, force_level=self.eng.last_jitter_level)
        W = torch.linalg.solve_triangular(L, self.kfun(self.Z, X), upper=False).T
        u, S = self.u, self.S
        if not self.whiten:
            u = torch.linalg.solve_triangular(L, u.T, upper=False).T
            S = torch.linalg.solve_triangular(L[None], S, upper=False)
        R = self.kfun(X, X) - W @ W.T
        T = W[None] @ S
        return u @ W.T, R, R[None] + T @ T.transpose(1, 2), W, u, S

    def restate_samples(self, X, xi, zeta, j, mean=None):
        loc, R, C, W, u, S = self.restate(X)
        G = torch.linalg.cholesky(R + j * torch.eye(X.shape[0], dtype=torch.float64))
        v = u[None] + (S[None] @ xi.double()[..., None])[..., 0]                  # (S, K, M)
        f = v @ W.T + zeta.double() @ G.T
        return f if mean is None else f + mean[None]


FIGS = {}


def note(key, val):
    FIGS[key] = max(FIGS.get(key, 0.0), val)
    print(f"{key}: {val:.3e} (largest so far {FIGS[key]:.3e})")


def check_cov(case, ns, label):
    eng = case.eng
    for n in ns:
        X = case.rows(n)
        full = eng.predict_cov(case.dev(X), 0).cpu()
        res = eng.predict_cov(case.dev(X), 1).cpu()
        _, R, C, *_ = case.restate(X)
        assert full.shape == (case.K, n, n) and res.shape == (n, n)
        assert torch.equal(full, full.transpose(1, 2)) and torch.equal(res, res.T)
        ec = relerr(full.numpy(), C.numpy())
        er = float((res.double() - R).abs().max() / C.abs().max())             # R is nearly 0 near the inducing points: relative to max |C| too
        note(f"cov {label} {case.dtype}", ec)
        note(f"resid {label} {case.dtype}", er)
        assert ec < TOL[case.dtype] and er < TOL[case.dtype], (n, ec, er)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("M", [12, 32])
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_covariance_against_the_restatement(kernel, M, K, whiten, dtype):
    check_cov(Case(kernel, M, K, dtype, whiten=whiten), NS_COV, kernel)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kernel", ["ard", "periodic", "product"])
def test_covariance_ard_periodic_and_product(kernel, dtype):
    check_cov(Case(kernel, 12, 3, dtype), (17, 65), kernel)


# ---- the model surface: the grid model M = 20 of the Monte-Carlo tests, perturbed parameters
NPTS = (5, 4)


def mean_fn(K):
    def f(x):
        k = torch.arange(K, dtype=x.dtype, device=x.device)[:, None]
        return (0.7 - 0.5 * k) * x[None, :, 0] + 0.4 * (k - 1.0) * x[None, :, 1] ** 2
    return f


def model_numbers(K, n, dtype, seed=0, twin=None):
    """the rows, counts, u and unconstrained S of model_case, drawn in its order; no device.  twin: the last row is the one before it
    moved by that much along axis 0 (the last row's entry of the factor of R then leans on the 32 columns before it)"""
    M = int(np.prod(NPTS))
    g = torch.Generator().manual_seed(100 * K + n + seed)
    xs = torch.rand(n, 2, generator=g, dtype=torch.float64)
    if twin and n > 1:
        xs[-1] = xs[-2] + torch.tensor([twin if float(xs[-2, 0]) < 0.5 else -twin, 0.0], dtype=torch.float64)
    xs = rnd(xs, dtype)
    ws = torch.randint(0, 5, (n, V), generator=g, dtype=torch.int32)
    u = rnd(0.5 * torch.randn(K, M, generator=g, dtype=torch.float64), dtype)
    s_unc = 0.1 * torch.randn(K, M, M, generator=g, dtype=torch.float64).tril(-1)
    s_unc = rnd(s_unc + torch.diag_embed(torch.full((K, M), math.log(0.3), dtype=torch.float64)), dtype)
    return xs, ws, u, s_unc


def model_case(K, n, dtype, mean=False, link_function=None, jitter=None, maxjitter=15, seed=0, ls=0.3, kernel="rbf", pure=False, twin=None):
    """(model, case): a SparseMultinomialGDRF holding n rows and a Case-shaped restatement of its numbers"""
    from gdrf_amd import kernels
    from gdrf_amd.models import SparseMultinomialGDRF
    xs, ws, u, s_unc = model_numbers(K, n, dtype, seed, twin)
    jit = JIT[dtype] if jitter is None else jitter
    kern = {"rbf": kernels.RBF, "matern52": kernels.Matern52}[kernel]
    model = SparseMultinomialGDRF(xs=xs.to(dtype), ws=ws, world=[(0.0, 1.0)] * 2, num_observation_categories=V,
                                  kernel=kern(input_dim=2, lengthscale=torch.tensor(ls), variance=torch.tensor(25.0)),
                                  num_topic_categories=K, dirichlet_param=0.01, n_points=list(NPTS), fixed_inducing_points=True,
                                  inducing_init="grid", jitter=jit, maxjitter=maxjitter, dtype=dtype, seed=5, device="cuda:0",
                                  link_function=link_function, mean_function=mean_fn(K) if mean else None, pure_fp32=pure)
    eng = model._engine
    assert eng.M == u.shape[1]
    case = Case.__new__(Case)
    case.kernel, case.M, case.K, case.dtype, case.whiten, case.D, case.eng = kernel, eng.M, K, dtype, True, 2, eng
    case.pure, case.span, case.jitter, case.s_unc, case.grid = pure, 1.0, jit, s_unc, None
    case.Z = eng.Z.detach().cpu().double()
    case.u = u
    case.S = s_unc.tril(-1) + torch.diag_embed(s_unc.diagonal(dim1=1, dim2=2).exp())
    eng.view("u_loc").copy_(case.u)
    eng.view("u_scale_tril_unc").copy_(s_unc)
    case.hyp = dict(log_lengthscale=eng.view("log_lengthscale").detach().cpu().double(), log_variance=eng.view("log_variance").detach().cpu().double())
    return model, case, xs, ws


def test_structure_of_the_covariance():
    """float64: symmetric to the bit; its diagonal is forward()'s var where mode 4's clamp is inactive; posterior's loc is forward's;
    no C_k has an eigenvalue below -1e-9 max |C|"""
    dtype, K, n = torch.float64, 3, 65
    model, case, xs, _ = model_case(K, n, dtype, mean=True, ls=0.08)      # a short lengthscale: no row sits on an inducing point
    loc, cov = model.posterior(xs)
    floc, fvar = model.forward(xs)
    assert cov.shape == (K, n, n) and torch.equal(cov, cov.transpose(1, 2))
    assert torch.equal(loc, floc)
    R = model._engine.predict_cov(case.dev(xs), 1)
    assert float(R.diagonal().min()) > 0.0, "mode 4's clamp of variance - |w|^2 must be inactive for this comparison"
    d = relerr(cov.diagonal(dim1=1, dim2=2).cpu().numpy(), fvar.cpu().numpy())
    note("diag vs forward var", d)
    assert d < 1e-9
    ev = torch.linalg.eigvalsh(cov.cpu()).min(dim=1).values / cov.abs().max().cpu()
    note("most negative eigenvalue / max|C|", float((-ev).max()))
    assert float(ev.min()) >= -1e-9
    rloc, _, C, *_ = case.restate(xs)
    assert relerr(cov.cpu().numpy(), C.numpy()) < TOL[dtype]
    assert relerr(loc.cpu().numpy(), (rloc + mean_fn(K)(xs)).numpy()) < TOL[dtype]
    with pytest.raises(NotImplementedError, match=r"posterior\(Xnew\) returns"):
        model.forward(xs, full_cov=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [1, 3])
def test_samples_with_injected_normals(K, dtype):
    """n at the Cholesky's 32-column panel edges, and one n past 256 rows: nine panels, every one still within the first 256-column chunk of
    the panel update (the second chunk needs n > 288; tests/test_gpu_joint_edges.py has those shapes)"""
    g = torch.Generator().manual_seed(3)
    for n in (1, 31, 32, 33, 257):
        model, case, xs, _ = model_case(K, n, dtype, mean=True)
        for S in (1, 3):
            xi = rnd(torch.randn(S, K, case.M, generator=g, dtype=torch.float64), dtype)
            zeta = rnd(torch.randn(S, K, n, generator=g, dtype=torch.float64), dtype)
            f = model.sample_fields(xs, S, xi=xi, zeta=zeta).cpu()
            assert f.shape == (S, K, n) and bool(torch.isfinite(f).all())
            want = case.restate_samples(xs, xi, zeta, case.eng.last_joint_jitter, mean_fn(K)(xs))
            e = relerr(f.numpy(), want.numpy())
            note(f"samples {dtype}", e)
            assert e < TOL[dtype], (n, S, e)
        zero = model.sample_fields(xs, 1, xi=torch.zeros(1, K, case.M), zeta=torch.zeros(1, K, n))[0]
        assert relerr(zero.cpu().numpy(), model.forward(xs)[0].cpu().numpy()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_samples_unwhitened_with_injected_normals(kernel, dtype):
    """whiten=False: the sampler reads L^-1 u_k and L^-1 S_k; engine level, M = 12 (the Mp padding), a topic-dependent mean"""
    K, M, S = 3, 12, 3
    case = Case(kernel, M, K, dtype, whiten=False, n_cap=65)
    g = torch.Generator().manual_seed(5)
    for n in (33, 65):
        X = case.rows(n)
        xi = rnd(torch.randn(S, K, M, generator=g, dtype=torch.float64), dtype)
        zeta = rnd(torch.randn(S, K, n, generator=g, dtype=torch.float64), dtype)
        mean = rnd(mean_fn(K)(X), dtype)
        f = case.eng.sample_joint(case.dev(X), S, xi=case.dev(xi), zeta=case.dev(zeta), mean=case.dev(mean)).cpu()
        e = relerr(f.numpy(), case.restate_samples(X, xi, zeta, case.eng.last_joint_jitter, mean).numpy())
        note(f"samples unwhitened {dtype}", e)
        assert e < TOL[dtype], (n, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_philox_draws(dtype):
    from gdrf_amd.engine import JOINT_XI_OFFSET, JOINT_ZETA_OFFSET
    K, n, S = 3, 33, 3
    model, case, xs, _ = model_case(K, n, dtype, mean=True)
    eng = model._engine
    a = model.sample_fields(xs, S, seed=11)
    assert torch.equal(a, model.sample_fields(xs, S, seed=11))
    assert not torch.equal(a, model.sample_fields(xs, S, seed=12))
    assert torch.equal(model.sample_fields(xs, S), model.sample_fields(xs, S, seed=model.rng_seed))
    # the documented keying: sample s of xi / zeta is what fill_eps writes for step = s on the stream's offset
    xi = torch.stack([eng.fill_eps(11, s, JOINT_XI_OFFSET, case.M) for s in range(S)]).contiguous()
    zeta = torch.stack([eng.fill_eps(11, s, JOINT_ZETA_OFFSET, n) for s in range(S)]).contiguous()
    assert xi.shape == (S, K, case.M) and zeta.shape == (S, K, n)
    assert torch.equal(a, model.sample_fields(xs, S, xi=xi, zeta=zeta))
    assert torch.equal(a, model.sample_fields(xs, S, seed=11, zeta=zeta)) and torch.equal(a, model.sample_fields(xs, S, seed=11, xi=xi))
    if dtype == torch.float64:                                          # (rounded to float32, two of a few hundred normals may coincide)
        both = torch.cat([xi.flatten(), zeta.flatten()])
        assert both.unique().numel() == both.numel()                    # no xi draw equals a zeta draw (nor another xi draw)
    # topic maps: the softmax of the field samples; rows sum to one within a few ulps
    maps = model.sample_topic_maps(xs, S, seed=11)
    assert maps.shape == (S, n, K)
    assert relerr(maps.cpu().numpy(), torch.softmax(a.double(), 1).transpose(1, 2).cpu().numpy()) < 16 * torch.finfo(dtype).eps
    assert float((maps.double().sum(-1) - 1).abs().max()) <= 4 * K * torch.finfo(dtype).eps
    link = lambda mu: torch.sigmoid(mu) / 2
    linked, _, _, _ = model_case(K, n, dtype, mean=True, link_function=link)
    lf = linked.sample_fields(xs, S, seed=11)
    assert torch.equal(lf, a)
    assert torch.equal(linked.sample_topic_maps(xs, S, seed=11), torch.stack([link(lf[s]).T for s in range(S)]))


def test_distribution_of_the_samples():
    """n = 6, K = 2, S = 4096, float64, fixed seed: every entry of the sample mean within 6 standard errors sqrt(C_ii / S) of loc, every entry
    of the sample covariance within 6 standard errors sqrt((C_ii C_jj + C_ij^2) / S) of C_k + j I.  Largest ratio seen: DESIGN.md section 19."""
    dtype, K, n, S = torch.float64, 2, 6, 4096
    model, case, xs, _ = model_case(K, n, dtype)
    f = model.sample_fields(xs, S, seed=20240229).cpu()                                # (S, K, n)
    loc, _, C, *_ = case.restate(xs)
    C = C + case.eng.last_joint_jitter * torch.eye(n, dtype=torch.float64)
    d = C.diagonal(dim1=1, dim2=2)                                                      # (K, n)
    zm = ((f.mean(0) - loc).abs() / (d / S).sqrt()).max()
    c = f - f.mean(0, keepdim=True)
    emp = torch.einsum("ski,skj->kij", c, c) / S
    zc = ((emp - C).abs() / ((d[:, :, None] * d[:, None, :] + C ** 2) / S).sqrt()).max()
    note("distribution: mean ratio", float(zm))
    note("distribution: covariance ratio", float(zc))
    assert float(zm) <= 6.0 and float(zc) <= 6.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jitter_loop_on_a_singular_residual(dtype):
    """Rows that hold every inducing point twice, and 20 other rows twice: R is singular, and with a first jitter of 1e-18 - below the
    rounding of R - the first level fails on a pivot the kernel flags; the call retries up the schedule.  A schedule of one level, or none,
    raises."""
    K, S = 2, 3
    model, case, xs0, _ = model_case(K, 80, dtype, jitter=1e-18)
    eng = model._engine
    xs = torch.cat([case.Z, case.Z, xs0[:20], xs0[:20]])
    f = model.sample_fields(xs, S, seed=4)
    note(f"jitter level {dtype}", eng.last_joint_level)
    assert eng.last_joint_level > 0 and eng.last_joint_jitter == eng.jitter_total(eng.last_joint_level) > eng.jitter_total(0)
    assert f.shape == (S, K, 80) and bool(torch.isfinite(f).all())
    # the retries redo only what depends on the jitter: the result is bit for bit a whole call on the level that was settled on
    from gdrf_amd import _lib
    whole, xd = torch.empty_like(f), case.dev(xs)
    _lib.check(eng.lib.gdrf_sample_joint(eng.ctx, xd.data_ptr(), 80, eng.Z.data_ptr(), eng.params.data_ptr(), S, 4, None, None,
                                         eng.last_joint_jitter, whole.data_ptr(), torch.cuda.current_stream(eng.device).cuda_stream),
               "gdrf_sample_joint")
    assert torch.equal(whole, f)
    assert eng.last_jitter_level == 0          # K_uu itself factorises on the first level: what fails below is R's pivot
    eng.maxjitter = 1
    with pytest.raises(RuntimeError, match="1 jitter levels"):
        model.sample_fields(xs, S, seed=4)
    eng.maxjitter = 0
    with pytest.raises(RuntimeError):
        model.sample_fields(xs, S, seed=4)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_side_effects_and_snapshot(dtype):
    K, n = 3, 63
    model, case, xs, ws = model_case(K, n, dtype, mean=True)
    eng = model._engine
    xd, wd = case.dev(xs), ws.to(eng.device)
    eps = case.dev(torch.randn(K, n, generator=torch.Generator().manual_seed(4), dtype=torch.float64))

    def step():
        eng.loss_and_grads(xd, wd, eps)
        return eng.out_d.clone(), eng.grads.clone()

    step()
    out1, g1 = step()
    loc, cov = model.posterior(xs[:40])
    f = model.sample_fields(xs[:40], 2)
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)
    # a snapshot restored from a saved and loaded checkpoint offers the same methods and returns what the live model returns, to the bit
    buf = io.BytesIO()
    torch.save({"model": copy.deepcopy(model)}, buf)
    buf.seek(0)
    snap = torch.load(buf, weights_only=False)["model"]
    for name in ("posterior", "sample_fields", "sample_topic_maps"):
        assert callable(getattr(snap, name))
    restored = snap.restore(mean_function=mean_fn(K))
    rloc, rcov = restored.posterior(xs[:40])
    assert torch.equal(rloc, loc) and torch.equal(rcov, cov)
    assert torch.equal(restored.sample_fields(xs[:40], 2), f)
    assert torch.equal(restored.sample_topic_maps(xs[:40], 2), model.sample_topic_maps(xs[:40], 2))


def test_limits():
    case = Case("rbf", 12, 2, torch.float64, n_cap=16)
    with pytest.raises(ValueError, match="n_cap"):
        case.eng.predict_cov(case.dev(case.rows(17)), 0)
    with pytest.raises(ValueError, match="n_cap"):
        case.eng.sample_joint(case.dev(case.rows(17)), 2, seed=1)
    with pytest.raises(ValueError, match="seed"):
        case.eng.sample_joint(case.dev(case.rows(8)), 2)
    assert case.eng.last_joint_jitter is None
