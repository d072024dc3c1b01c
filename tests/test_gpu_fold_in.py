"""GPU tests of the fold-in path (gdrf_fold_in, csrc/foldin.h) against a float64 torch restatement of its definition and of the iteration
it is judged against, both written here.  For row n, with m = f_loc + mean and s = f_var + noise (the location and scale of the model's
mu site), counts w, R = sum w, theta = softmax(mu), p = theta Phi:

    J(mu) = sum_{v: w_v > 0} w_v log p_v - 1/2 sum_k ((mu_k - m_k) / s_k)^2,      mu_hat = a local maximiser reached from mu = m
    g_k = r_k - R theta_k - (mu_k - m_k) / s_k^2,   r_k = theta_k sum_v w_v Phi_kv / p_v

The iteration (``iterate``): E-step r at mu, then two Newton steps on Q(mu') = r . mu' - R lse(mu') - prior(mu') by Sherman-Morrison, the
step capped at max |delta| = 4 and halved up to 12 times until Q does not decrease; the difference Q(mu + t delta) - Q(mu) is evaluated as
q . td - R (log1p(sum_k theta_k expm1(td_k)) - theta . td) - 1/2 sum_k td_k^2 / s_k^2 (td = t delta, q the gradient of Q at mu).

The model is that of tests/test_gpu_predict_mc.py (grid model M = 20, perturbed parameters; float32 contexts compared at float32-valued
parameters), its tolerances TOL too: 1e-9 in fp64 contexts, 5e-4 in float32 ones, relerr = max-abs over max-abs.  For the property tests
m and s are the device's own predict mode 4 and noise, cast to float64 (their parity with the oracle is pinned by test_gpu_parity.py);
test_model_methods_tie_to_the_oracle takes them from the oracle's conditional instead.  Row totals 3000, 0, 1, 20 alternate in every call.

|g|_inf / max(1, R) is a difference of O(1) terms: precision bounds its absolute error.  It is compared as max-abs over max-abs at 0, 1 and
4 iterations, where its largest value is O(0.1) (not for K = 1 or V = 1, where g is zero in exact arithmetic), and absolutely (the
issue's "+ TOL") at every count.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from tests._util import dev, relerr
from tests._mc_util import MEAN_KN, NPTS, build, engine, loc_var

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-9, torch.float32: 5e-4}
DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
NS = (1, 63, 257)
NT = 63                    # rows of the checks against the float64 iteration (its two thousand iterations run on the host)
# (K, V): every lane-group form of the kernel (8, 16, 32, 64 lanes, two topics per lane above 64), the 16- and 64-lane ones at both ends; every V
CASES = [(1, 9), (2, 1), (5, 9), (9, 9), (16, 64), (17, 64), (33, 9), (64, 65), (65, 65), (128, 64)]
CASE_IDS = [f"K{k}-V{v}" for k, v in CASES]
TOTALS = (3000, 0, 1, 20)
CAP, INNER, HALVINGS = 4.0, 2, 12


# ---- the definition and the iteration, float64 ---------------------------------------------------------------------------------
def jg(mu, w, Phi, m, s):
    """J (n,), r (n, K), theta (n, K), R (n, 1) and g (n, K) of the definition at mu (n, K)"""
    th = torch.softmax(mu, -1)
    p = th @ Phi
    pos = w > 0
    J = torch.where(pos, w * torch.where(pos, p, torch.ones_like(p)).log(), torch.zeros_like(p)).sum(-1) - 0.5 * (((mu - m) / s) ** 2).sum(-1)
    c = torch.where(pos, w / p, torch.zeros_like(p))
    r = th * (c @ Phi.T)
    R = w.sum(-1, keepdim=True)
    return J, r, th, R, r - R * th - (mu - m) / s ** 2


def gnorm(mu, w, Phi, m, s):
    _, _, _, R, g = jg(mu, w, Phi, m, s)
    return g.abs().amax(-1) / R[:, 0].clamp(min=1.0)


def m_step(mu, r, th, R, m, is2):
    """the two capped, line-searched Newton steps on Q from mu (theta = softmax(mu), r the E-step's counts): the new mu.  numpy arrays"""
    cur, alive = mu.copy(), np.ones(mu.shape[0], dtype=bool)
    for _ in range(INNER):
        q = r - R * th - (cur - m) * is2
        D = R * th + is2
        sa, den = (th * q / D).sum(-1, keepdims=True), (th * is2 / D).sum(-1, keepdims=True)
        dl = (q + th * (R * sa / den)) / D
        dmax = np.abs(dl).max(-1, keepdims=True)
        alive = alive & (dmax[:, 0] > 0)
        t = np.where(dmax > CAP, CAP / np.maximum(dmax, 1e-300), 1.0)
        acc = np.zeros_like(alive)
        t_acc, th_acc = np.zeros_like(t), th.copy()
        for _ in range(HALVINGS + 1):
            td = t * dl
            ex = th * np.expm1(td)
            u = ex.sum(-1, keepdims=True)
            lin = (td * (q - 0.5 * is2 * td)).sum(-1)
            ok = (lin - R[:, 0] * (np.log1p(u[:, 0]) - (th * td).sum(-1)) >= 0) & ~acc & alive
            t_acc = np.where(ok[:, None], t, t_acc)
            th_acc = np.where(ok[:, None], (th + ex) / (1.0 + u), th_acc)
            acc = acc | ok
            if (acc | ~alive).all():
                break
            t = t * 0.5
        cur = np.where(acc[:, None], cur + t_acc * dl, cur)
        th = np.where(acc[:, None], th_acc, th)
        alive = alive & acc                          # no step accepted: the second try from the same point would give the same
    return cur


def iterate(w, Phi, m, s, iters, keep=()):
    """mu after `iters` iterations from mu = m (tol = 0); `keep`: iteration counts whose mu is returned as well, {count: mu}.  A row that
    an iteration leaves where it was is left there by every later one (the iteration has no state but mu): such rows leave the work.
    float64 tensors in and out, numpy inside (two thousand iterations of small arrays)."""
    w, Phi, m, s = (x.double().numpy() for x in (w, Phi, m, s))
    mu, is2, out = m.copy(), 1.0 / s ** 2, {}
    act = np.arange(mu.shape[0])
    pos = w > 0
    R = w.sum(-1, keepdims=True)
    for it in range(iters + 1):
        if it in keep:
            out[it] = torch.from_numpy(mu.copy())
        if it == iters:
            break
        if act.size == 0:
            out.update({k: torch.from_numpy(mu.copy()) for k in keep if k > it})
            break
        ma = mu[act]
        e = np.exp(ma - ma.max(-1, keepdims=True))
        th = e / e.sum(-1, keepdims=True)
        c = np.where(pos[act], w[act] / np.where(pos[act], th @ Phi, 1.0), 0.0)
        r = th * (c @ Phi.T)
        cur = m_step(ma, r, th, R[act], m[act], is2[act])
        mu[act] = cur
        act = act[(cur != ma).any(-1)]
    mu = torch.from_numpy(mu)
    return (mu, out) if keep else mu


def counts(n, V, seed):
    """(n, V) int32 counts whose row totals run through TOTALS, each row from its own word distribution"""
    rng = np.random.default_rng(seed)
    w = np.zeros((n, V), dtype=np.int32)
    for i in range(n):
        p = np.exp(1.5 * rng.standard_normal(V))
        w[i] = rng.multinomial(TOTALS[i % 4], p / p.sum())
    return torch.from_numpy(w)


class Case:
    """One (K, V, dtype): the engine, 257 rows with their counts, (m, s) of the device in float64 and, on demand, the float64 iteration"""

    def __init__(self, K, V, dtype, n=max(NS), **kw):
        self.K, self.V, self.dtype, self.n = K, V, dtype, n
        self.m_ = build(K, n, dtype, V=V, **kw)
        self.eng = engine(self.m_, dtype)
        self.xs = dev(self.m_.xs, self.eng)
        self.w = counts(n, V, 100 * K + V)
        self.wd = dev(self.w, self.eng, torch.int32)
        self.w64 = self.w.double()
        with torch.no_grad():
            self.Phi = self.m_.constrained()["phi"].double()
        self._traj = None

    @property
    def ms(self):
        """(m, s), each (n, K) float64, from the device's predict mode 4 and noise"""
        if not hasattr(self, "_ms"):
            lv = self.eng.predict(self.xs, 4).double().cpu()
            noise = float(self.eng.view("log_noise").exp().double().cpu())
            self._ms = lv[0].T.contiguous(), (lv[1] + noise).T.contiguous()
        return self._ms

    def traj(self):
        """the float64 iteration's mu of the first NT rows at 64 and 400 iterations and at 2000 (J*), computed once"""
        if self._traj is None:
            m, s = self.ms
            star, kept = iterate(self.w64[:NT], self.Phi, m[:NT], s[:NT], 2000, keep=(64, 400))
            self._traj = dict(kept, star=star)
        return self._traj

    def fold(self, mode, iters, tol=0.0, n=None, ws=None, **kw):
        n = self.n if n is None else n
        out, diag = self.eng.fold_in(self.xs[:n], self.wd[:n] if ws is None else ws, mode, iters, tol, **kw)
        return out.double().cpu(), diag.cpu()

    def J(self, mu):
        return jg(mu, self.w64[:mu.shape[0]], self.Phi, self.ms[0][:mu.shape[0]], self.ms[1][:mu.shape[0]])[0]


@functools.lru_cache(maxsize=None)
def case(K, V, dtype):
    return Case(K, V, dtype)


def both(f):
    return pytest.mark.parametrize("dtype", DTYPES, ids=IDS)(pytest.mark.parametrize("K,V", CASES, ids=CASE_IDS)(f))


# ---- 1
@both
def test_zero_iterations_is_the_plug_in(K, V, dtype):
    c = case(K, V, dtype)
    m, _ = c.ms
    for n in NS:
        th0, d0 = c.fold(0, 0, n=n)
        mu0, _ = c.fold(1, 0, n=n)
        assert th0.shape == (n, K) and mu0.shape == (K, n) and d0.shape == (3, n)
        assert relerr(th0.numpy(), c.eng.predict(c.xs[:n], 1).double().cpu().numpy()) < TOL[dtype]
        assert torch.equal(mu0.T, m[:n]) and bool((d0[2] == 0).all())
        th64, d64 = c.fold(0, 64, n=n)
        mu64, _ = c.fold(1, 64, n=n)
        empty = c.w64[:n].sum(-1) == 0
        assert torch.equal(th64[empty], th0[empty]) and torch.equal(mu64.T[empty], mu0.T[empty])
        if K == 1:
            assert bool((th64 == 1).all()) and bool((th0 == 1).all())
        assert bool((d64[2] <= 64).all())


# ---- 2
@both
def test_J_never_decreases_with_the_iterations(K, V, dtype):
    c = case(K, V, dtype)
    prev = None
    for iters in (0, 1, 2, 4, 8, 16, 64):
        mu, diag = c.fold(1, iters)
        J = c.J(mu.T.contiguous())
        slack = TOL[dtype] * J.abs().clamp(min=1.0)
        print(f"K={K} V={V} {dtype} iters={iters} sum J={float(J.sum()):.6f} reported-recomputed={float(((diag[0] - J).abs() / J.abs().clamp(min=1.0)).max()):.2e}")
        assert bool(((diag[0] - J).abs() <= slack).all())                  # the reported J is J at the returned mu
        if prev is not None:
            assert bool((J >= prev - slack).all()), float((prev - J).max())
        prev = J
    if K > 1 and V > 1:
        assert bool((prev > c.J(c.ms[0]) + 1.0)[c.w64.sum(-1) >= 20].any())          # and it does move


# ---- 3
@both
def test_reaches_the_optimum_as_the_float64_iteration_does(K, V, dtype):
    c = case(K, V, dtype)
    t = c.traj()
    Js = c.J(t["star"])
    scale = Js.abs().clamp(min=1.0)
    gap_ref = (Js - c.J(t[64])) / scale
    mu, _ = c.fold(1, 64, n=NT)
    gap = (Js - c.J(mu.T.contiguous())) / scale
    print(f"K={K} V={V} {dtype} gap at 64: device max {float(gap.max()):.2e} min {float(gap.min()):.2e}, float64 iteration max {float(gap_ref.max()):.2e}")
    assert bool((gap_ref >= -1e-12).all())
    assert bool((gap <= 4 * gap_ref + TOL[dtype]).all()), float((gap - 4 * gap_ref).max())


# ---- 4
@both
def test_stationarity_is_reported_and_reached(K, V, dtype):
    c = case(K, V, dtype)
    m, s = c.ms
    m, s, w = m[:NT], s[:NT], c.w64[:NT]
    for iters in (0, 1, 4, 64, 400):
        mu, diag = c.fold(1, iters, n=NT)
        g = gnorm(mu.T.contiguous(), w, c.Phi, m, s)
        print(f"K={K} V={V} {dtype} iters={iters} |g|/R reported max {float(diag[1].max()):.3e} recomputed max {float(g.max()):.3e} "
              f"abs diff {float((diag[1] - g).abs().max()):.2e}")
        if iters <= 4 and K > 1 and V > 1:
            assert relerr(diag[1].numpy(), g.numpy()) < TOL[dtype]
        assert bool(((diag[1] - g).abs() <= TOL[dtype]).all())
    g_ref = gnorm(c.traj()[400], w, c.Phi, m, s)
    print(f"K={K} V={V} {dtype} |g|/R at 400: device max {float(g.max()):.2e}, float64 iteration max {float(g_ref.max()):.2e}")
    assert bool((g <= 4 * g_ref + TOL[dtype]).all()) and bool((diag[1] <= 4 * g_ref + TOL[dtype]).all())


# ---- 5
@both
def test_tol_stops_a_row_once_its_gradient_is_small(K, V, dtype):
    c = case(K, V, dtype)
    _, full = c.fold(1, 64, tol=0.0)
    for tol in (1e-2, 1e-4):
        for iters in (3, 64):
            _, d = c.fold(1, iters, tol=tol)
            used, g = d[2], d[1]
            assert bool((used <= iters).all()) and bool((used >= 0).all()) and bool((used == used.round()).all())
            assert bool((g[used < iters] <= tol).all())
            assert bool((used <= full[2]).all())
        if K > 1 and V > 1:
            assert bool((used < full[2]).any())              # some row did stop early at 64


# ---- 6
@both
def test_counts_and_scores_follow_from_the_returned_theta(K, V, dtype):
    c = case(K, V, dtype)
    tol = TOL[dtype]
    th, _ = c.fold(0, 16)
    mu, _ = c.fold(1, 16)
    r, _ = c.fold(2, 16)
    assert relerr(th.numpy(), torch.softmax(mu.T, -1).numpy()) < tol
    assert float((th.sum(-1) - 1).abs().max()) <= 4 * K * float(torch.finfo(dtype).eps)
    p = th @ c.Phi
    pos = c.w64 > 0
    r_ref = th * (torch.where(pos, c.w64 / p, torch.zeros_like(p)) @ c.Phi.T)
    R = c.w64.sum(-1)
    assert relerr(r.numpy(), r_ref.numpy()) < tol
    assert float((r.sum(-1) - R).abs().max()) / float(R.max()) < tol
    # The score's restatement takes the returned theta with its rows summing to one: a float32 theta sums to 1 within a few ulps
    # (asserted above), and that rounding, a relative error of p common to all the words of a row, would enter the restatement as
    # sum w x 6e-8 (2e5 counts here) - its own error, and all there is where log p = 0 (V = 1).
    pn = (th / th.sum(-1, keepdim=True)) @ c.Phi
    w2 = counts(c.n, V, 7 + K)
    for ws_score, w in ((None, c.w64), (dev(w2, c.eng, torch.int32), w2.double())):
        sc, _ = c.fold(3, 16, ws_score=ws_score)
        want = float(torch.where(w > 0, w * pn.log(), torch.zeros_like(pn)).sum())
        print(f"K={K} V={V} {dtype} score {float(sc[0]):.6f} want {want:.6f}")
        assert float(sc[1]) == float(w.sum())
        assert abs(float(sc[0]) - want) <= tol * max(1.0, abs(want))


# ---- 7
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,V", [(5, 9), (16, 9), (17, 64), (64, 64), (128, 64)], ids=["K5-V9", "K16-V9", "K17-V64", "K64-V64", "K128-V64"])
def test_results_do_not_depend_on_how_the_rows_are_batched(K, V, dtype):
    from gdrf_amd.data import csr_rows, to_csr
    c = case(K, V, dtype)
    ws_csr = to_csr(c.wd)
    for sparse in (False, True):
        for mode in (0, 1, 2):
            one, d1 = c.eng.fold_in(c.xs, ws_csr if sparse else c.wd, mode, 16, 1e-5)
            parts = [c.eng.fold_in(c.xs[a:a + 63], csr_rows(ws_csr, slice(a, a + 63)) if sparse else c.wd[a:a + 63], mode, 16, 1e-5)
                     for a in range(0, c.n, 63)]
            two = torch.cat([p[0] for p in parts], dim=1 if mode == 1 else 0)
            assert torch.equal(one, two) and torch.equal(d1, torch.cat([p[1] for p in parts], dim=1)), (sparse, mode)


# ---- 8
def with_stored_zero(w):
    """the CSR form of the dense counts w with one explicitly stored zero added (in the first row that has an absent word)"""
    n, V = w.shape
    crow, col, val = [0], [], []
    done = False
    for i in range(n):
        for v in range(V):
            x = int(w[i, v])
            if x != 0 or (not done and i > 0):
                done = done or x == 0
                col.append(v); val.append(x)
        crow.append(len(col))
    assert done
    return torch.sparse_csr_tensor(torch.tensor(crow, dtype=torch.int64), torch.tensor(col, dtype=torch.int64),
                                   torch.tensor(val, dtype=torch.int32), size=(n, V))


@both
def test_csr_counts_give_the_dense_results(K, V, dtype):
    from gdrf_amd.data import to_csr
    c = case(K, V, dtype)
    tol = TOL[dtype]
    n = 63
    sp = with_stored_zero(c.w[:n]).to(c.eng.device)
    assert sp.values().numel() == int((c.w[:n] != 0).sum()) + 1
    assert int((sp.crow_indices()[1:] == sp.crow_indices()[:-1]).sum()) > 0            # rows without entries
    for mode in (0, 1, 2):
        a, da = c.fold(mode, 16, n=n)
        b, db = c.fold(mode, 16, n=n, ws=sp)
        assert relerr(b.numpy(), a.numpy()) < tol, mode
        assert relerr(db[0].numpy(), da[0].numpy()) < tol and bool(((db[1] - da[1]).abs() <= tol).all())
    w2 = counts(n, V, 11 + K)
    a, _ = c.fold(3, 16, n=n, ws_score=dev(w2, c.eng, torch.int32))
    b, _ = c.fold(3, 16, n=n, ws=sp, ws_score=to_csr(dev(w2, c.eng, torch.int32)))
    assert float(a[1]) == float(b[1]) and abs(float(a[0]) - float(b[0])) <= tol * max(1.0, abs(float(a[0])))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_large_sparse_vocabulary_runs_where_the_dense_form_refuses(dtype):
    from gdrf_amd._lib import GdrfHipError
    from gdrf_amd.data import to_csr
    K, V, n = 5, 2000, 63
    c = Case(K, V, dtype, n=n)
    rng = np.random.default_rng(5)
    w = np.zeros((n, V), dtype=np.int32)
    for i in range(n):
        cols = rng.choice(V, size=40, replace=False)                       # 2 % of the words
        w[i, cols] = rng.multinomial(TOTALS[i % 4], np.full(40, 1 / 40))
    c.w, c.w64 = torch.from_numpy(w), torch.from_numpy(w).double()
    c.wd = dev(c.w, c.eng, torch.int32)
    sp = to_csr(c.wd)
    with pytest.raises(GdrfHipError, match="too large"):
        c.fold(0, 4)
    m, s = c.ms
    prev = None
    for iters in (0, 4, 32):
        mu, diag = c.fold(1, iters, ws=sp)
        J, g = c.J(mu.T.contiguous()), gnorm(mu.T.contiguous(), c.w64, c.Phi, m, s)
        slack = TOL[dtype] * J.abs().clamp(min=1.0)
        assert bool(((diag[0] - J).abs() <= slack).all()) and bool(((diag[1] - g).abs() <= TOL[dtype]).all())
        if iters <= 4:
            assert relerr(diag[1].numpy(), g.numpy()) < TOL[dtype]
        assert prev is None or bool((J >= prev - slack).all())
        prev = J
    star, kept = iterate(c.w64, c.Phi, m, s, 400, keep=(32,))
    scale = c.J(star).abs().clamp(min=1.0)
    assert bool(((c.J(star) - J) / scale <= 4 * (c.J(star) - c.J(kept[32])) / scale + TOL[dtype]).all())


# ---- 9
def _model(m, dtype, n_cap, kind="rbf", whiten=True, mean_function=None):
    """A SparseMultinomialGDRF with the oracle's parameters and inducing inputs whose engine holds n_cap rows"""
    from gdrf_amd.kernels import KERNEL_DICT
    from gdrf_amd.models import SparseMultinomialGDRF
    model = SparseMultinomialGDRF(xs=m.xs[:n_cap], ws=m.ws[:n_cap], world=[(0.0, 1.0)] * 2, num_observation_categories=m.V,
                                  kernel=KERNEL_DICT[kind](input_dim=2, lengthscale=torch.tensor(0.3), variance=torch.tensor(25.0)),
                                  num_topic_categories=m.K, dirichlet_param=0.01, n_points=list(NPTS), fixed_inducing_points=True,
                                  inducing_points=m.Z, jitter=m.jitter, maxjitter=15, dtype=dtype, seed=5, device="cuda:0",
                                  mean_function=mean_function, whiten=whiten)
    for name in model._engine.PARAM_NAMES:
        model._engine.view(name).copy_(m.params[name].detach().to(dtype))
    return model


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["mean_function", "unwhitened", "matern52"])
def test_model_methods_tie_to_the_oracle(variant, dtype, monkeypatch):
    import gdrf_amd.models.sparse_gdrf as sg
    from gdrf_amd.data import to_csr
    K, V, n, tol = 5, 9, 257, TOL[dtype]
    mean_fn = MEAN_KN if variant == "mean_function" else None
    kind = "matern52" if variant == "matern52" else "rbf"
    m = build(K, n, dtype, kind=kind, whiten=variant != "unwhitened", mean_function=mean_fn)
    model = _model(m, dtype, n, kind=kind, whiten=variant != "unwhitened", mean_function=mean_fn)
    xs, w, w2 = m.xs.to(dtype), counts(n, V, 3), counts(n, V, 4)
    mu0 = model.infer_log_topic_probs(xs, w, num_iters=0)
    m.force_jitter_level = model._engine.last_jitter_level
    loc, var = loc_var(m, m.xs)                                             # the oracle's conditional, mean_function added
    with torch.no_grad():
        Phi, noise = m.constrained()["phi"].double(), float(m.constrained()["noise"])
    mo, so = loc.T.contiguous(), (var + noise).T.contiguous()
    assert mu0.shape == (K, n) and relerr(mu0.double().cpu().numpy(), loc.numpy()) < tol
    assert relerr(model.infer_topic_probs(xs, w, num_iters=0).double().cpu().numpy(), torch.softmax(mo, -1).numpy()) < tol
    # the optimum of the oracle's own objective is reached as its float64 iteration reaches it
    w64 = w.double()[:NT]
    star, kept = iterate(w64, Phi, mo[:NT], so[:NT], 2000, keep=(64,))
    Jo = lambda mu: jg(mu[:NT], w64, Phi, mo[:NT], so[:NT])[0]
    scale = Jo(star).abs().clamp(min=1.0)
    mu, diag = model.infer_log_topic_probs(xs, w, num_iters=64, tol=0.0, return_diagnostics=True)
    assert diag.shape == (3, n) and diag.dtype == torch.float64
    gap, gap_ref = (Jo(star) - Jo(mu.double().cpu().T.contiguous())) / scale, (Jo(star) - Jo(kept[64])) / scale
    print(f"{variant} {dtype} gap device {float(gap.max()):.2e} float64 iteration {float(gap_ref.max()):.2e}")
    assert bool((gap <= 4 * gap_ref + tol).all())
    assert relerr(diag[0][:NT].cpu().numpy(), Jo(mu.double().cpu().T.contiguous()).numpy()) < tol
    # the methods agree with each other, dense and CSR, in one call and in pieces, on the model and on a restored snapshot
    th = model.infer_topic_probs(xs, w, num_iters=64, tol=0.0)
    r = model.topic_counts(xs, w, num_iters=64, tol=0.0)
    assert th.shape == (n, K) and r.shape == (n, K) and relerr(th.double().cpu().numpy(), torch.softmax(mu.double().cpu().T, -1).numpy()) < tol
    p = th.double().cpu() @ Phi
    want = math.exp(-float(torch.where(w2 > 0, w2.double() * p.log(), torch.zeros_like(p)).sum()) / float(w2.sum()))
    ppl = model.completion_perplexity(xs, w, w2, num_iters=64, tol=0.0)
    assert ppl.dim() == 0 and abs(float(ppl) - want) / want < tol
    ppl_csr = model.completion_perplexity(xs, to_csr(w), to_csr(w2), num_iters=64, tol=0.0)
    assert abs(float(ppl_csr) - want) / want < tol
    assert relerr(model.infer_topic_probs(xs, to_csr(w), num_iters=64, tol=0.0).double().cpu().numpy(), th.double().cpu().numpy()) < tol
    snap = copy.deepcopy(model)
    restored = snap.restore(mean_function=mean_fn)
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 80)          # the restored model's engine grows to at most 80 rows: pieces
    for name, ref in (("infer_topic_probs", th), ("infer_log_topic_probs", mu), ("topic_counts", r)):
        assert callable(getattr(snap, name))
        assert torch.equal(getattr(restored, name)(xs, w, num_iters=64, tol=0.0), ref), name
        assert torch.equal(getattr(restored, name)(xs, to_csr(w), num_iters=64, tol=0.0), getattr(model, name)(xs, to_csr(w), num_iters=64, tol=0.0))
    assert restored._engine.n_cap == 80
    ppl_p, d_p = restored.completion_perplexity(xs, w, w2, num_iters=64, tol=0.0, return_diagnostics=True)
    assert abs(float(ppl_p) - want) / want < tol and d_p.shape == (3, n)
    if mean_fn is None:
        assert torch.equal(snap.infer_topic_probs(xs, w, num_iters=64, tol=0.0), th)


# ---- 10
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fold_in_is_closer_to_the_truth_than_the_plug_in(dtype):
    K, V, n = 10, 50, 257
    c = Case(K, V, dtype, n=n)
    m, s = c.ms
    g = torch.Generator().manual_seed(20240229)
    th_true = torch.softmax(m + s * torch.randn(n, K, generator=g, dtype=torch.float64), -1)
    p = th_true @ c.Phi
    rng = np.random.default_rng(9)
    w = torch.from_numpy(np.stack([rng.multinomial(1000, (pi / pi.sum()).numpy()) for pi in p]).astype(np.int32))
    plug = float((torch.softmax(m, -1) - th_true).abs().mean())
    ref = float((torch.softmax(iterate(w.double(), c.Phi, m, s, 64), -1) - th_true).abs().mean())
    th, _ = c.fold(0, 64, tol=1e-6, ws=dev(w, c.eng, torch.int32))
    got = float((th - th_true).abs().mean())
    print(f"{dtype} mean |theta - theta_true|: plug-in {plug:.4f} float64 iteration {ref:.4f} device {got:.4f}")
    assert ref < plug
    assert got < plug


def test_limits():
    m = build(5, 63, torch.float64)
    eng = engine(m, torch.float64, n_cap=32)
    xs, ws = dev(m.xs, eng), dev(counts(63, 9, 1), eng, torch.int32)
    with pytest.raises(ValueError, match="n_cap"):
        eng.fold_in(xs, ws, 0)
    with pytest.raises(ValueError, match="num_iters"):
        eng.fold_in(xs[:32], ws[:32], 0, num_iters=-1)
    with pytest.raises(ValueError, match="int32"):
        eng.fold_in(xs[:32], ws[:32].to(torch.int64), 0)
    assert eng.fold_in(xs[:32], ws[:32].contiguous(), 0)[0].shape == (32, 5)
