"""GPU: the joint posterior and the batch choice (csrc/predict_cov.h, csrc/select_batch.h, chol_kernel of csrc/kernels_mm.h as the n x n
factorisation) past the shapes of tests/test_gpu_joint.py and tests/test_gpu_select_batch.py, which all have Mp = 32, n <= 257 rows to
factorise, at most 9 (sample, topic) rows, D <= 2 and a float64 solve:

  M = 33, 64, 65, 257   Mp = 64, 64, 96, 288: a second round of every loop over Mp, a block with one real column, a block count that is odd,
                        a second round of 256 threads / a second workgroup along Mp
  n = 288, 289, 545, 1057 rows to factorise: chol_kernel's second column chunk, second strip group (545 in double, 1057 in float) and
                        stage (c)'s second round
  S K = 63, 64, 65, 129 the 64-row tiles of joint_sample_kernel
  D = 3, 4              the GDRF_DMAX loops of the residual's epilogue and of the pass
  the all-fp32 context  Impl<float, float>: every kernel above on float vectors of four and the float matrix instruction

The shapes, their inputs and what each crosses are tests/_joint_ref.py's lists (tests/test_joint_edges_host.py recomputes the crossings and
shows that the measures see a skipped block of W or a skipped part of the factorisation).  The float64 and float32 contexts are held
against the float64 torch restatements of the two files above with their assertions and their bounds, 1e-7 and 1e-4.  The all-fp32 context
is held against the np.longdouble restatement of tests/_joint_ref.py with the bound computed there, 64 err(float32 restatement) + 2^-23,
at most 5e-4; the batch choice takes the case's bound for C_k.

Largest figures seen on an MI355X are recorded in DESIGN.md sections 19 and 23."""
import numpy as np
import pytest
import torch

import tests.test_gpu_joint as J
import tests.test_gpu_select_batch as SB
from tests import _joint_ref as R
from tests._util import relerr

pytestmark = pytest.mark.gpu

if not R.P.HAS_LONGDOUBLE:
    pytest.skip("np.longdouble has no more precision than float64 here: the exact restatement needs eps < 1e-18", allow_module_level=True)

BY = {name: R._list(name) for name in ("cov", "select", "sample")}
pairs = lambda name: [(e["id"], ctx) for e in BY[name].values() for ctx in e["ctxs"]]


def engine_case(e, ctx, n_cap):
    case = R.make_case(e, ctx, n_cap=n_cap, engine=True)
    assert case.eng.pure_fp32 == (ctx == "pure")
    return case


def pure_reference(case, name, id, n, X):
    """(exact, bounds) of an all-fp32 case; the host's inputs are the device's, and both stand on the first jitter level"""
    inp, exact, b = R.pure_reference(R.engine_inputs, name, id, "pure", n)
    assert np.array_equal(inp["X"], X.numpy()) and np.array_equal(inp["Z"], case.eng.Z.cpu().double().numpy())
    assert max(b.values()) <= R.CEILING
    return exact, b


def held(key, err, bound):
    J.note(key, err)
    J.note(key + " / bound", err / bound)
    return err <= bound


# ---- covariance -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("id,ctx", pairs("cov"))
def test_covariance(id, ctx):
    e = BY["cov"][id]
    case = engine_case(e, ctx, max(e["ns"]))
    if ctx != "pure":
        J.check_cov(case, e["ns"], "edges " + id)
        return
    eng = case.eng
    for n in e["ns"]:
        X = case.rows(n)
        full = eng.predict_cov(case.dev(X), 0).cpu()
        res = eng.predict_cov(case.dev(X), 1).cpu()
        assert eng.last_jitter_level == 0
        exact, b = pure_reference(case, "cov", id, n, X)
        assert full.shape == (case.K, n, n) and res.shape == (n, n)
        assert torch.equal(full, full.transpose(1, 2)) and torch.equal(res, res.T)
        m = R.measures(dict(C=full.numpy(), R=res.numpy()), exact)
        ok = [held("cov edges pure", m["C"], b["C"]), held("resid edges pure", m["R"], b["R"])]
        assert all(ok), (n, m, b)


# ---- samples ----------------------------------------------------------------------------------------------------------------------------

def sample_model(K, n, ctx):
    model, case, xs, _ = J.model_case(K, n, R.torch_dtype(ctx), mean=True, jitter=R.MODEL_JITTER[ctx], ls=R.MODEL_LS[ctx], kernel="matern52",
                                      pure=ctx == "pure", twin=R.TWIN)
    eng = model._engine
    assert eng.pure_fp32 == (ctx == "pure") and eng.M == int(np.prod(R.MODEL_GRID))
    ll, lv = R.model_hyp(ctx)                        # the hyper-parameters as values the element type holds: the host's numbers
    eng.view("log_lengthscale").copy_(ll)
    eng.view("log_variance").copy_(lv)
    case.hyp = dict(log_lengthscale=ll, log_variance=lv)
    return model, case, xs


def check_samples(K, S, n, ctx):
    """test_samples_with_injected_normals' assertions on one (K, S, n)"""
    model, case, xs = sample_model(K, n, ctx)
    dtype, eng = case.dtype, case.eng
    xi, zeta = R.normals(S, K, case.M, n, dtype)
    f = model.sample_fields(xs, S, xi=xi, zeta=zeta).cpu()
    assert f.shape == (S, K, n) and bool(torch.isfinite(f).all())
    zero = model.sample_fields(xs, 1, xi=torch.zeros(1, K, case.M), zeta=torch.zeros(1, K, n))[0].cpu()
    fwd = model.forward(xs)[0].cpu()
    if ctx != "pure":
        want = case.restate_samples(xs, xi, zeta, eng.last_joint_jitter, J.mean_fn(K)(xs))
        err = relerr(f.numpy(), want.numpy())
        J.note(f"samples edges {dtype}", err)
        assert err < J.TOL[dtype], (n, S, err)
        assert relerr(zero.numpy(), fwd.numpy()) < J.TOL[dtype]
        return
    inp, exact, b = R.pure_reference(R.model_inputs, K, S, n, "pure")
    assert np.array_equal(inp["X"], xs.numpy()) and np.array_equal(inp["Z"], eng.Z.cpu().double().numpy())
    assert eng.last_jitter_level == 0 and eng.last_joint_level == 0 and eng.last_joint_jitter == inp["jrow"]
    assert max(b.values()) <= R.CEILING
    assert held("samples edges pure", R.measures(dict(f=f.numpy()), exact)["f"], b["f"]), (n, S, b)
    assert held("zero draw edges pure", R.measures(dict(f0=zero.numpy()), exact)["f0"], b["f0"]), (n, b)
    assert relerr(zero.numpy(), fwd.numpy()) <= 2 * b["f0"]


@pytest.mark.parametrize("n,ctx", [(n, ctx) for ctx in R.CTXS for n in R.SAMPLE_N[ctx]])
def test_samples_past_the_first_chunk_of_the_factorisation(n, ctx):
    """K = 1, S = 2, M = 20: what each n reaches in chol_kernel is tests/_joint_ref.py's SAMPLE_N_EXPECT"""
    check_samples(1, 2, n, ctx)


@pytest.mark.parametrize("ctx", R.CTXS)
@pytest.mark.parametrize("K,S", R.SAMPLE_SK)
def test_samples_at_the_tile_edges_of_the_sample_rows(K, S, ctx):
    check_samples(K, S, R.SAMPLE_SK_N, ctx)


@pytest.mark.parametrize("id,ctx", pairs("sample"))
def test_samples_at_257_inducing_points(id, ctx):
    """engine level, whitened and not: joint_v_kernel's second workgroup along Mp, nine 32-column blocks in both sample products"""
    e = BY["sample"][id]
    n, S, K = 65, e["S"], e["K"]
    case = engine_case(e, ctx, n)
    X = case.rows(n)
    xi, zeta = R.normals(S, K, case.M, n, case.dtype)
    f = case.eng.sample_joint(case.dev(X), S, xi=case.dev(xi), zeta=case.dev(zeta)).cpu()
    assert f.shape == (S, K, n) and bool(torch.isfinite(f).all())
    if ctx != "pure":
        err = relerr(f.numpy(), case.restate_samples(X, xi, zeta, case.eng.last_joint_jitter).numpy())
        J.note(f"samples edges M = 257 {case.dtype}", err)
        assert err < J.TOL[case.dtype], err
        return
    exact, b = pure_reference(case, "sample", id, n, X)
    assert case.eng.last_jitter_level == 0 and case.eng.last_joint_level == 0
    assert held("samples edges M = 257 pure", R.measures(dict(f=f.numpy()), exact)["f"], b["f"]), b


@pytest.mark.parametrize("ctx", R.CTXS)
def test_philox_draws_at_257_inducing_points_and_129_sample_rows(ctx):
    """the seeded call equals the call given its own fill_eps draws, bit for bit (test_philox_draws' keying)"""
    from gdrf_amd.engine import JOINT_XI_OFFSET, JOINT_ZETA_OFFSET
    e = R.PHILOX_CASE
    n, S, K = 65, e["S"], e["K"]
    case = engine_case(e, ctx, n)
    eng, X = case.eng, case.dev(case.rows(n))
    a = eng.sample_joint(X, S, seed=11)
    assert a.shape == (S, K, n) and bool(torch.isfinite(a).all())
    assert torch.equal(a, eng.sample_joint(X, S, seed=11)) and not torch.equal(a, eng.sample_joint(X, S, seed=12))
    xi = torch.stack([eng.fill_eps(11, s, JOINT_XI_OFFSET, case.M) for s in range(S)]).contiguous()
    zeta = torch.stack([eng.fill_eps(11, s, JOINT_ZETA_OFFSET, n) for s in range(S)]).contiguous()
    assert xi.shape == (S, K, case.M) and zeta.shape == (S, K, n)
    assert torch.equal(a, eng.sample_joint(X, S, xi=xi, zeta=zeta))
    assert torch.equal(a, eng.sample_joint(X, S, seed=11, zeta=zeta)) and torch.equal(a, eng.sample_joint(X, S, seed=11, xi=xi))


# ---- batch choice -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("id,ctx", pairs("select"))
def test_batch_choice(id, ctx):
    e = BY["select"][id]
    G = e["given"]
    case = engine_case(e, ctx, max(e["ns"]) + G)
    given = case.rows(G, seed=77, near=False) if G else None
    for n in e["ns"]:
        count = min(n, R.COUNT)
        X = SB.rows_with_a_gap(case, n, count, given=given)
        if ctx != "pure":
            SB.check(case, X, count, given=given, label="edges " + id)
            continue
        _, b = pure_reference(case, "select", id, n, X if given is None else torch.cat([X, given]))
        SB.check(case, X, count, given=given, label="edges pure", tol=b["C"])
        assert case.eng.last_jitter_level == 0
