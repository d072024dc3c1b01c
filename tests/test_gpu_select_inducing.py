"""GPU tests of the greedy choice of inducing points (gdrf_select_inducing, csrc/select_inducing.h) against tests/_inducing_ref.py, a float64
restatement of its definition: the loop, and diag(K_nn - K_nP K_PP^-1 K_Pn) by a dense solve.

Bounds, relative to k(x, x): tests/test_gpu_joint.py's, 1e-7 in float64 contexts and 1e-4 with float32 arrays (the f64 solve); the all-fp32
context gets 4 (G + count) eps32, the rounding of a history sum of G + count products each bounded by the variance.  A float32 context is
compared at the same float32-valued rows and log-parameters.  The floor is (G + count) eps(solve type) k(x, x), what the model passes.

The greedy-consistency check, in every case: at each step the restatement is conditioned on the DEVICE's earlier picks; the device's pick
must have a reference d within the bound of the reference's largest, and the returned pivot, trace (per row) and final residual must equal
the reference's within the bound (a near-tie may flip an argmax, nothing else).  Pivots and trace never increase, picks are distinct.  In the
float64 cases of _inducing_ref.EXACT_CASES the picks must equal the restatement's own greedy run.

Largest figures seen on an MI355X are recorded in DESIGN.md section 27."""
import copy
import io

import numpy as np
import pytest
import torch

from tests import _inducing_ref as R

pytestmark = pytest.mark.gpu

CTXS = ["fp64", "fp32", "pure"]
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
FIGS = {}
ENGINES = {}


def note(key, val):
    FIGS[key] = max(FIGS.get(key, 0.0), val)
    print(f"{key}: {val:.3e} (largest so far {FIGS[key]:.3e})")


class Ctx:
    """One engine of the context type ``ctx`` ("fp64"; "fp32": float32 arrays with the f64 solve; "pure": all fp32) with the kernel
    ``kind`` at the parameters of the restatement's Kern.  The engines are kept: a test that asks for the same one gets it again."""

    def __init__(self, kind, ctx, D=2, ls=0.3, n_cap=1200):
        from gdrf_amd.engine import Engine
        self.ctx, self.D = ctx, D
        self.dtype = torch.float64 if ctx == "fp64" else torch.float32
        self.kern = R.Kern(kind, D, "float64" if ctx == "fp64" else "float32", ls=ls)
        key = (kind, ctx, D, ls, n_cap)
        if key not in ENGINES:
            name, kw = self.kern.engine_kwargs()
            eng = Engine(n_cap, 4, 1, 2, D, dtype=self.dtype, kernel=name, process_group=None, pure_fp32=ctx == "pure", **kw)
            for k, v in self.kern.log.items():
                view = eng.view(k)
                view.copy_(torch.as_tensor(v).reshape(view.shape))
            ENGINES[key] = eng
        self.eng = ENGINES[key]
        self.eps = EPS32 if ctx == "pure" else EPS64

    def rows(self, seed, n):
        """uniform rows of the unit cube that the context's element type holds exactly"""
        return R.uniform_rows(seed, n, self.D).astype(np.float32 if self.dtype == torch.float32 else np.float64).astype(np.float64)

    def dev(self, a):
        return torch.as_tensor(np.asarray(a)).to(device=self.eng.device, dtype=self.dtype).contiguous()

    def tol(self, T):
        return {"fp64": 1e-7, "fp32": 1e-4, "pure": 4 * T * EPS32}[self.ctx]

    def floor(self, T):
        return T * self.eps * self.kern.variance

    def run(self, X, count, given=None):
        G = 0 if given is None else len(given)
        out = self.eng.select_inducing(self.dev(X), count, given=None if given is None else self.dev(given), floor=self.floor(G + count),
                                       return_residual=True)
        idx, piv, tr, rank, resid = out
        assert idx.dtype == torch.int64 and piv.dtype == tr.dtype == resid.dtype == torch.float64 and isinstance(rank, int)
        assert idx.shape == (count,) and piv.shape == tr.shape == (G + count,) and resid.shape == (len(X),)
        return idx.cpu().numpy(), piv.cpu().numpy(), tr.cpu().numpy(), rank, resid.cpu().numpy()


def check(c, X, count, given=None, label="", exact=False):
    """run the engine on the rows X and hold the result against the restatement conditioned on its picks; returns what the engine returned"""
    n, G = len(X), 0 if given is None else len(given)
    T, var = G + count, c.kern.variance
    tol, floor = c.tol(T), c.floor(T)
    idx, piv, tr, rank, resid = c.run(X, count, given)
    assert np.isfinite(piv).all() and np.isfinite(tr).all() and np.isfinite(resid).all()
    picks = idx.tolist()
    assert all(0 <= p < n for p in picks) and len(set(picks)) == count, picks
    ref = R.greedy(c.kern, X, count, given=given, floor=floor, forced=picks)
    figs = dict(short=float(((ref["best"] - ref["pivots"][G:]) / var).max()) if count else 0.0,
                pivot=float(np.abs(piv - ref["pivots"]).max() / var), trace=float(np.abs(tr - ref["trace"]).max() / (n * var)),
                resid=float(np.abs(resid - ref["d"]).max() / var))
    for k, v in figs.items():
        note(f"{k} {label} {c.ctx}", v)
    assert all(v < tol for v in figs.values()), (figs, tol)
    assert np.all(np.diff(piv[G:]) <= tol * var), piv                               # the free picks' pivots never increase
    assert np.all(np.diff(tr) <= tol * n * var) and tr[0] <= n * c.kern.diag() * (1 + 1e-12), tr   # nor does the trace
    # the rank: every reference pivot clearly above the floor counts, none clearly below does
    assert int((ref["pivots"] > floor + tol * var).sum()) <= rank <= int((ref["pivots"] > floor - tol * var).sum()), (rank, ref["rank"])
    if exact:
        own = R.greedy(c.kern, X, count, given=given, floor=floor)
        assert own["gap"] >= R.EXACT_GAP * var, own["gap"]
        assert picks == own["picks"], (picks, own["picks"])
    return idx, piv, tr, rank, resid


# every row edge of the pass: one row, the 64-lane wave, the 256-row tile, two tiles and a row
@pytest.mark.parametrize("ctx", CTXS)
def test_row_edges(ctx):
    c = Ctx("rbf", ctx)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        check(c, c.rows(n, n), min(n, 9), label="rows")


@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("count", [1, 7, 8, 9, 17])
def test_counts_across_the_history_unroll(count, ctx):
    """a call with count picks runs every history length 0 .. count - 1: one short of a round of eight, a round, a round and one, two and one"""
    c = Ctx("rbf", ctx)
    check(c, c.rows(3, 65), count, label="counts")


@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("n", [1, 65, 257])
def test_every_row_picked(n, ctx):
    """count = n: a permutation, and with the Exponential kernel at ls 0.2 every pivot is far above the floor: rank = n"""
    c = Ctx("exponential", ctx, ls=0.2)
    idx, piv, _, rank, resid = check(c, c.rows(4, n), n, label="count = n")
    assert sorted(idx.tolist()) == list(range(n)) and rank == n
    assert np.abs(resid).max() < c.tol(n) * c.kern.variance                        # nothing is left of a row that is a point itself


@pytest.mark.parametrize("ctx", CTXS)
def test_given_rows(ctx):
    c = Ctx("rbf", ctx)
    X, given = c.rows(5, 65), c.rows(77, 3)
    _, piv, tr, _, _ = check(c, X, 9, given=given, label="given")
    _, free, trf, _, _ = check(c, X, 9, label="given")
    assert piv[3] <= free[0] and tr[2] < trf[0]                                      # conditioning on more cannot raise a pivot
    # count = 0: the coverage of an existing set; no index comes back
    idx, piv0, tr0, rank, _ = check(c, X, 0, given=given, label="count = 0")
    assert idx.size == 0 and rank == 3 and np.array_equal(piv0, piv[:3]) and np.array_equal(tr0, tr[:3])
    # a given of no rows is no given, to the bit
    a = c.eng.select_inducing(c.dev(X), 9, given=c.dev(np.zeros((0, 2))), floor=c.floor(9), return_residual=True)
    b = c.eng.select_inducing(c.dev(X), 9, floor=c.floor(9), return_residual=True)
    assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("ctx", CTXS)
def test_300_picks_of_700_rows(ctx):
    """past gdrf_select_batch's 256 picks; the preparation gathers the pivot's history with more than one entry per thread"""
    c = Ctx("matern32", ctx, ls=0.1)
    _, _, _, rank, _ = check(c, c.rows(6, 700), 300, label="300 picks")
    assert rank == 300


def test_the_cap_of_1024_picks():
    from gdrf_amd.engine import INDUCING_MAX_PICKS
    c = Ctx("exponential", "fp64", ls=0.1)
    X, given = c.rows(7, 1100), c.rows(78, 3)
    _, _, _, rank, _ = check(c, X, INDUCING_MAX_PICKS - 3, given=given, label="1024 picks")
    assert rank == INDUCING_MAX_PICKS
    with pytest.raises(ValueError, match="INDUCING_MAX_PICKS"):
        c.eng.select_inducing(c.dev(X), INDUCING_MAX_PICKS - 2, given=c.dev(given))
    with pytest.raises(ValueError, match="n_cap"):
        c.eng.select_inducing(c.dev(c.rows(1, 1199)), 2, given=c.dev(given))


@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernels(kind, ctx):
    c = Ctx(kind, ctx, D=1 if kind == "periodic" else 2)
    check(c, c.rows(8, 65), 9, given=c.rows(79, 2), label=kind)


@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_dimensions(D, ctx):
    for kind in ("matern52", "ard"):
        c = Ctx(kind, ctx, D=D)
        check(c, c.rows(9, 65), 9, label=f"D = {D}")
    if D <= 2:
        c = Ctx("periodic", ctx, D=D)
        check(c, c.rows(9, 65), 9, label=f"D = {D}")


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: f"seed{c[0]}-{c[4]}")
def test_exact_picks_in_float64(case):
    seed, n, D, M, kind, ls = case
    c = Ctx(kind, "fp64", D=D, ls=ls)
    _, _, _, rank, _ = check(c, R.uniform_rows(seed, n, D), M, label="exact", exact=True)
    assert rank == M


@pytest.mark.parametrize("ctx", CTXS)
def test_duplicates(ctx):
    """40 distinct rows, each three times: rank 40, the first 40 picks are 40 different places, each the lowest index of its three, and the
    last 10 pivots are at most the floor"""
    c = Ctx("rbf", ctx, ls=0.2)
    a = c.rows(11, 40)
    X = np.concatenate([a, a, a])
    idx, piv, _, rank, _ = check(c, X, 50, label="duplicates")
    assert rank == 40 and sorted(idx[:40].tolist()) == list(range(40))
    assert piv[40:].max() <= c.floor(50)
    # a given row twice: the second is a degenerate pick and changes nothing
    g = c.rows(12, 1)
    once, twice = c.run(X[:40], 4, given=g), c.run(X[:40], 4, given=np.concatenate([g, g]))
    assert twice[3] == once[3] == 5 and twice[1][1] <= c.floor(6) and np.array_equal(once[0], twice[0])


def test_ties_go_to_the_lower_index():
    """every d starts as the same number: the first pick is row 0; on cat(a, a) each later pick lies in the first half while its twin is free"""
    c = Ctx("rbf", "fp64")
    a = c.rows(13, 65)
    idx = c.run(np.concatenate([a, a]), 9)[0].tolist()
    assert idx[0] == 0
    for t, p in enumerate(idx):
        assert p < 65 or (p - 65) in idx[:t], (t, idx)


def test_striding_workgroups_and_the_two_stage_argmax():
    """2048 x 256 + 257 rows: more tiles than workgroups, a last tile of one row.  All rows but the LAST lie in a small box, the last one far
    from it: after row 0 (the tie of equal d) the best row is the last row of the last tile"""
    from gdrf_amd.engine import Engine
    n = 2048 * 256 + 257
    kern = R.Kern("rbf", 2, ls=0.3)
    X = 0.4 + 0.1 * R.uniform_rows(14, n, 2)
    X[-1] = (0.98, 0.97)
    eng = Engine(n, 4, 1, 2, 2, dtype=torch.float64, kernel="rbf", process_group=None)
    for k, v in kern.log.items():
        eng.view(k).copy_(torch.as_tensor(v))
    floor = 4 * EPS64 * kern.variance
    idx, piv, tr, rank, resid = eng.select_inducing(torch.as_tensor(X).to(eng.device), 4, floor=floor, return_residual=True)
    picks = idx.tolist()
    assert picks[:2] == [0, n - 1] and rank == 4
    ref = R.greedy(kern, X, 4, floor=floor, forced=picks)
    assert np.abs(ref["best"] - ref["pivots"]).max() < 1e-7 * kern.variance
    assert np.abs(piv.cpu().numpy() - ref["pivots"]).max() < 1e-7 * kern.variance
    assert np.abs(tr.cpu().numpy() - ref["trace"]).max() < 1e-7 * n * kern.variance
    assert np.abs(resid.cpu().numpy() - ref["d"]).max() < 1e-7 * kern.variance


@pytest.mark.parametrize("ctx", CTXS)
def test_bit_identical_calls(ctx):
    c = Ctx("matern52", ctx)
    X, given = c.dev(c.rows(15, 700)), c.dev(c.rows(80, 3))
    same = lambda a, b: all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))
    a = c.eng.select_inducing(X, 40, given=given, floor=c.floor(43), return_residual=True)
    assert same(a, c.eng.select_inducing(X, 40, given=given, floor=c.floor(43), return_residual=True))
    other = Ctx("exponential", ctx, ls=0.2)
    other.run(other.rows(16, 257), 20)
    assert same(a, c.eng.select_inducing(X, 40, given=given, floor=c.floor(43), return_residual=True))


@pytest.mark.parametrize("ctx", CTXS)
def test_mesh_against_greedy_on_a_track(ctx):
    """the device's trace of the 6 x 6 mesh (count = 0, given = mesh) and of 36 greedy picks each match the dense solve, and greedy leaves
    less than half of what the mesh leaves (on the CPU: 0.034 against 0.330 of n var)"""
    c = Ctx("rbf", ctx, ls=0.1)
    f32 = lambda a: a.astype(np.float32).astype(np.float64) if ctx != "fp64" else a
    X, mesh = f32(R.spiral_track()), f32(R.mesh(6))
    scale, tol = 600 * c.kern.variance, c.tol(36)
    _, _, tr_mesh, rank_mesh, d_mesh = check(c, X, 0, given=mesh, label="track, mesh")
    idx, _, tr, rank, d = check(c, X, 36, label="track, greedy")
    assert rank_mesh == rank == 36
    print(f"residual trace / (n var) {ctx}: mesh {tr_mesh[-1] / scale:.4f}, greedy {tr[-1] / scale:.4f}")
    for got_tr, got_d, P in ((tr_mesh[-1], d_mesh, mesh), (tr[-1], d, X[idx])):
        dense = R.nystrom_residual(c.kern, X, P)
        assert abs(got_tr - dense.sum()) < tol * scale and np.abs(got_d - dense).max() < tol * c.kern.variance
    assert tr[-1] < 0.5 * tr_mesh[-1]


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
V, NPTS = 3, (5, 4)


def model_rows(n=90, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 2, generator=g, dtype=torch.float64), torch.randint(0, 5, (n, V), generator=g, dtype=torch.int32)


def build(xs, ws, world=((0.0, 1.0), (0.0, 1.0)), **kw):
    from gdrf_amd import kernels
    from gdrf_amd.models import SparseMultinomialGDRF
    args = dict(xs=xs, ws=ws, world=list(world), num_observation_categories=V,
                kernel=kernels.Matern52(input_dim=2, lengthscale=torch.tensor(0.3), variance=torch.tensor(25.0)), num_topic_categories=2,
                dirichlet_param=0.01, n_points=list(NPTS), fixed_inducing_points=True, inducing_init="greedy", jitter=1e-6, maxjitter=15,
                dtype=torch.float64, seed=5, device="cuda:0")
    args.update(kw)
    return SparseMultinomialGDRF(**args)


def one_step(model, xs, ws):
    from gdrf_amd import poutine
    from gdrf_amd.infer import SVI, Trace_ELBO
    from gdrf_amd.optim import Adam
    scale = poutine.scale(scale=1.0 / len(xs))
    svi = SVI(model=scale(model.model), guide=scale(model.guide), optim=Adam({"lr": 1e-2}),
              loss=Trace_ELBO(max_plate_nesting=1, vectorize_particles=True, num_particles=1))
    return svi.step(xs=xs.to(model.device), ws=ws.to(model.device), subsample=False)


@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "learnable"])
def test_greedy_initialisation_of_the_model(fixed):
    xs, ws = model_rows()
    model = build(xs, ws, fixed_inducing_points=fixed)
    M = NPTS[0] * NPTS[1]
    res = model.choose_inducing_points(xs)                                           # count = M, at the hyper-parameters still initial
    assert res["rank"] == M and res["indices"].shape == (M,) and res["pivots"].shape == res["residual_trace"].shape == (M,)
    want = xs[res["indices"].cpu()]
    assert torch.equal(res["points"].cpu(), want)
    Z = model.inducing_points.cpu()
    assert torch.equal(Z, want) if fixed else float((Z - want).abs().max()) < 1e-12   # learnable: sigmoid(logit(z)), a few ulp of 1
    assert Z.unique(dim=0).shape[0] == M
    loss = one_step(model, xs, ws)
    assert np.isfinite(loss)
    # deep copy and snapshot restore keep the points and do not select again (restore has no candidates to select from)
    Z = model.inducing_points.cpu().clone()
    buf = io.BytesIO()
    torch.save({"model": copy.deepcopy(model)}, buf)
    buf.seek(0)
    snap = torch.load(buf, weights_only=False)["model"]
    assert callable(snap.choose_inducing_points)
    restored = snap.restore()
    assert torch.equal(restored.inducing_points.cpu(), Z)
    # engine growth keeps them too
    more, _ = model_rows(200, seed=22)
    model.choose_inducing_points(more, count=3)                                      # all rows in one call: a larger engine
    assert model._engine.n_cap >= 200 and torch.equal(model.inducing_points.cpu(), Z)


def test_candidates_of_their_own_a_scaled_world_and_thinning():
    xs, ws = model_rows()
    world = ((0.0, 2.0), (-1.0, 1.0))
    cand, _ = model_rows(150, seed=23)
    cand = cand * torch.tensor([2.0, 2.0], dtype=torch.float64) + torch.tensor([0.0, -1.0], dtype=torch.float64)
    model = build(xs, ws, world=world, inducing_candidates=cand)
    res = model.choose_inducing_points(cand, return_residual=True)
    assert res["residual"].shape == (150,)
    want = cand[res["indices"].cpu()]
    assert torch.equal(res["points"].cpu(), want)
    assert torch.equal(model.inducing_points.cpu(), model.scale(want))                # the scaled rows
    # the coverage of the model's own points: their scaled coordinates mapped back to the world
    own = model.inducing_points.cpu() * torch.tensor([2.0, 2.0], dtype=torch.float64) + torch.tensor([0.0, -1.0], dtype=torch.float64)
    cover = model.choose_inducing_points(cand, count=0, given=own)
    assert cover["indices"].numel() == 0 and cover["rank"] == 20
    assert abs(float(cover["residual_trace"][-1]) - float(res["residual_trace"][-1])) < 1e-7 * 150 * 25.0
    # thinning: 150 rows looked at as the rows floor(i 150 / 40); the indices refer to cand
    thin = model.choose_inducing_points(cand, count=7, max_candidates=40, return_residual=True)
    rows = [i * 150 // 40 for i in range(40)]
    sub = model.choose_inducing_points(cand[rows], count=7)
    assert thin["residual"].shape == (40,) and thin["indices"].tolist() == [rows[i] for i in sub["indices"].tolist()]
    assert torch.equal(thin["points"].cpu(), cand[thin["indices"].cpu()]) and torch.equal(thin["pivots"], sub["pivots"])


def test_fewer_distinct_places_than_points_raises():
    xs, ws = model_rows()
    few = xs[:12].repeat(5, 1)                                                        # 60 candidates, 12 places, M = 20
    with pytest.raises(ValueError, match="only 12 distinct places"):
        build(xs, ws, inducing_candidates=few)


def test_train_passes_the_method_through():
    from gdrf_amd.train import train
    xs, ws = model_rows(60)
    out = train(xs=xs.numpy(), ws=ws.numpy(), dimensions=2, epochs=2, num_topics=2, num_inducing_points=[3, 3],
                inducing_initialization_method="greedy", kernel_lengthscale=0.3, fixed_inducing_points=True)
    model = out["model"]
    Z = model.inducing_points.cpu()
    S = model.scale(xs.float()).cpu()
    assert Z.shape == (9, 2) and np.isfinite(out["history"][:, 0]).all()
    assert all(bool(((S - z).abs().max(1).values < 1e-6).any()) for z in Z)            # every inducing point is a row of the data
