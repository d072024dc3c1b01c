"""GPU tests of the greedy batch choice (gdrf_select_batch, csrc/select_batch.h) against tests/_select_ref.py, a float64 restatement of its
definition by dense solves on the columns C_k[:, A].

Bounds: tests/test_gpu_joint.py's bounds for C_k, 1e-7 in float64 contexts and 1e-4 in float32 ones, applied to the gains relative to the
first gain and to the variances relative to the largest prior variance.  A float32 context is compared at the same float32-valued
parameters, rows and inducing inputs, on the jitter level the engine reports.

The greedy-consistency check, in every case: at each step the restatement is conditioned on the DEVICE's earlier picks; the device's pick
must have a reference gain within the bound of the reference's largest, and the returned gain must equal that reference gain within the
bound (a near-tie may flip an argmax, nothing else).  In float64 contexts the picks must, in addition, equal the restatement's own greedy run
at every step: the rows come from the first of 20 seeds whose relative gap between the best and the second-best reference gain is at least
1e-5 at every step, 100 times the bound.

Largest figures seen on an MI355X are recorded in DESIGN.md section 23."""
import copy
import io

import pytest
import torch

import tests.test_gpu_joint as J
from tests._select_ref import SelectRef

pytestmark = pytest.mark.gpu

TOL = J.TOL
DTYPES, IDS = J.DTYPES, J.IDS
GAP = 1e-5
S2 = 0.37
FIGS = {}


def note(key, val):
    FIGS[key] = max(FIGS.get(key, 0.0), val)
    print(f"{key}: {val:.3e} (largest so far {FIGS[key]:.3e})")


def check(case, X, count, s2=S2, given=None, exact=None, label="", tol=None):
    """run the engine on the rows X and hold the result against the restatement; returns (idx, gains, var) on the CPU.  tol: the bound,
    where it is not the context's fixed one (the all-fp32 context: the case's computed bound for C_k)"""
    eng, dtype, n = case.eng, case.dtype, X.shape[0]
    tol = TOL[dtype] if tol is None else tol
    out = eng.select_batch(case.dev(X), count, s2, given=None if given is None else case.dev(given), return_variance=True)
    idx, gains, var = (t.cpu() for t in out)
    assert idx.dtype == torch.int64 and gains.dtype == torch.float64 and var.dtype == torch.float64
    assert idx.shape == (count,) and gains.shape == (count,) and var.shape == (case.K, n)
    assert bool(torch.isfinite(gains).all()) and bool(torch.isfinite(var).all())
    picks = idx.tolist()
    assert all(0 <= p < n for p in picks) and len(set(picks)) == count, picks
    ref = SelectRef(case, X, s2, given)
    g0 = float(ref.gains([]).max())
    for t in range(count):
        g = ref.gains(picks[:t])
        short = (float(g.max()) - float(g[picks[t]])) / g0
        err = abs(float(gains[t]) - float(g[picks[t]])) / g0
        note(f"pick shortfall {label} {dtype}", short)
        note(f"gain {label} {dtype}", err)
        assert short < tol and err < tol, (t, short, err)
    assert bool((gains[1:] <= gains[:-1] + tol * g0).all()), gains                     # submodular: the gains never increase
    d = ref.cond_var(picks)[:, :n]
    vmax = float(ref.diag.max())
    ev = float((var - d).abs().max()) / vmax
    note(f"variance {label} {dtype}", ev)
    assert ev < tol, ev
    total = abs(float(gains.sum()) - ref.information(picks)) / g0                      # sum_t gain_t = I(picked)
    note(f"sum of gains {label} {dtype}", total)
    assert total < count * tol, total
    if exact is None:
        exact = dtype == torch.float64
    if exact:
        want, _, gap = ref.greedy(count)
        assert gap >= GAP, gap
        assert picks == want, (picks, want)
    return idx, gains, var


def rows_with_a_gap(case, n, count, s2=S2, given=None):
    """the rows of the first of 20 seeds on which the restatement's own greedy run has a relative gap of at least GAP between the best and
    the second-best gain at every step (float64 contexts: the device must then pick the same rows); float32 contexts take the first seed"""
    case.eng.factorize()
    for seed in range(1, 21):
        X = case.rows(n, seed)
        if case.dtype != torch.float64 or SelectRef(case, X, s2, given).greedy(count)[2] >= GAP:
            return X
    raise AssertionError(f"no seed of 20 gives a gap of {GAP} at every step (n = {n}, count = {count})")


# every row edge of the pass: its 64-row tile (a lane group's four rows, two at a time, inside it), two tiles, a tile and a row
NS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_edges(dtype):
    case = J.Case("rbf", 12, 3, dtype, n_cap=257)
    for n in NS:
        count = min(n, 9)
        check(case, rows_with_a_gap(case, n, count), count, label="rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("K", [1, 3, 15, 16])
@pytest.mark.parametrize("M", [12, 32])
def test_topics_and_inducing_points(M, K, whiten, dtype):
    """K + 1 = 16 fills the block of right-hand sides, 17 starts a second one; M = 12 is padded to 32 columns"""
    case = J.Case("rbf", M, K, dtype, whiten=whiten, n_cap=65)
    check(case, rows_with_a_gap(case, 65, 9), 9, label="topics")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("kernel", ["matern52", "ard", "periodic", "product"])
def test_kernels(kernel, whiten, dtype):
    case = J.Case(kernel, 12, 3, dtype, whiten=whiten, n_cap=65)
    check(case, rows_with_a_gap(case, 65, 9), 9, label=kernel)


def test_128_topics():
    case = J.Case("rbf", 12, 128, torch.float64, n_cap=65)
    check(case, rows_with_a_gap(case, 65, 3), 3, label="K = 128")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("count", [1, 9, 33, 65])
def test_counts(count, dtype):
    """count = n returns a permutation (check() asserts distinct indices inside [0, n)).  The pass reads the history in rounds of eight
    entries with a tail: a call with count picks runs every history length 0 .. count - 1, so 9 covers the first full round and 33 and 65
    every remainder after one to eight of them"""
    case = J.Case("rbf", 12, 3, dtype, n_cap=65)
    idx, _, _ = check(case, rows_with_a_gap(case, 65, count), count, label="counts")
    if count == 65:
        assert sorted(idx.tolist()) == list(range(65))


def test_the_cap_of_256_picks():
    """G + count = SELECT_MAX_PICKS: the preparation gathers a history of 255 entries, one per thread"""
    from gdrf_amd.engine import SELECT_MAX_PICKS
    case = J.Case("rbf", 12, 1, torch.float64, n_cap=300)
    X = rows_with_a_gap(case, 257, SELECT_MAX_PICKS)
    check(case, X, SELECT_MAX_PICKS, label="256 picks")
    with pytest.raises(ValueError, match="SELECT_MAX_PICKS"):
        case.eng.select_batch(case.dev(X), SELECT_MAX_PICKS, S2, given=case.dev(case.rows(1)))
    with pytest.raises(ValueError, match="n_cap"):
        case.eng.select_batch(case.dev(case.rows(300)), 2, S2, given=case.dev(case.rows(1)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("G", [1, 5])
def test_given_rows(G, dtype):
    case = J.Case("rbf", 12, 3, dtype, n_cap=65 + G)
    given = case.rows(G, seed=77)
    X = rows_with_a_gap(case, 65, 9, given=given)
    _, gains, _ = check(case, X, 9, given=given, label="given")
    _, free, _ = check(case, X, 9, exact=False, label="given")
    assert float(gains[0]) <= float(free[0]) * (1 + TOL[dtype])    # conditioning on more cannot raise a gain
    # a given of no rows is no given, to the bit
    a = case.eng.select_batch(case.dev(X), 9, S2, given=case.dev(torch.zeros(0, case.D)), return_variance=True)
    b = case.eng.select_batch(case.dev(X), 9, S2, return_variance=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_given_of_no_rows_on_the_model():
    model, case, xs, _ = J.model_case(3, 65, torch.float64)
    a = model.select_batch(xs, 9, given=torch.zeros(0, 2))
    b = model.select_batch(xs, 9, given=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_known_answers_on_the_model(dtype):
    K, n, count = 3, 65, 9
    tol = TOL[dtype]
    model, case, xs, _ = J.model_case(K, n, dtype, ls=0.08)
    idx, gains, var = model.select_batch(xs, count, noise=S2, return_variance=True)
    assert idx.device == model._engine.device
    # sum(gains) = 1/2 sum_k logdet(I + C_k[sel, sel] / s2) with C_k from posterior()
    C = model.posterior(xs[idx.cpu()])[1].double().cpu()
    info = float(0.5 * torch.logdet(torch.eye(count, dtype=torch.float64)[None] + C / S2).sum())
    e = abs(float(gains.sum()) - info) / float(gains[0])
    note(f"sum of gains vs posterior {dtype}", e)
    assert e < count * tol
    assert bool((gains[1:] <= gains[:-1] + tol * gains[0]).all())
    assert idx.unique().numel() == count
    # the conditional variances are the restatement's and nowhere above forward()'s
    fvar = model.forward(xs)[1].double()
    ref = SelectRef(case, xs, S2)
    d = ref.cond_var(idx.tolist())
    assert float((var.cpu() - d).abs().max()) / float(ref.diag.max()) < tol
    assert bool((var <= fvar + tol * fvar.max()).all())
    # the default noise is the model's own parameter
    a = model.select_batch(xs, count)
    b = model.select_batch(xs, count, noise=float(model.noise))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_go_to_the_lower_index(dtype):
    """on cat(a, a) every row has a twin with the same gain, to the bit: each pick lies in the first half while its twin is free"""
    case = J.Case("rbf", 12, 3, dtype, n_cap=130)
    a = case.rows(65)
    X = torch.cat([a, a])
    idx, gains, _ = check(case, X, 9, exact=False, label="ties")
    first = idx.tolist()
    assert first[0] < 65
    for t, p in enumerate(first):
        assert p < 65 or (p - 65) in first[:t], (t, first)


def test_several_workgroups_and_the_two_stage_argmax():
    """n = 2^16 + 1 rows, 1025 tiles on 1024 workgroups; all rows but the LAST lie in a small box among the inducing points, the last one far
    from them: the best row is the last row of the last tile"""
    n, M, K = 2 ** 16 + 1, 32, 3
    g = torch.Generator().manual_seed(9)
    Z = 0.3 + 0.3 * torch.rand(M, 2, generator=g, dtype=torch.float64)
    case = J.Case("rbf", M, K, torch.float64, n_cap=n, Z=Z)
    X = 0.4 + 0.1 * torch.rand(n, 2, generator=g, dtype=torch.float64)
    X[-1] = torch.tensor([0.98, 0.97], dtype=torch.float64)
    case.eng.factorize()
    assert int(SelectRef(case, X, S2).gains([]).argmax()) == n - 1
    idx, _, _ = check(case, X, 4, exact=False, label="2^16 + 1 rows")
    assert int(idx[0]) == n - 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_side_effects_and_snapshot(dtype):
    K, n = 3, 63
    model, case, xs, ws = J.model_case(K, n, dtype, mean=True)
    eng = model._engine
    xd, wd = case.dev(xs), ws.to(eng.device)
    eps = case.dev(torch.randn(K, n, generator=torch.Generator().manual_seed(4), dtype=torch.float64))

    def step():
        eng.loss_and_grads(xd, wd, eps)
        return eng.out_d.clone(), eng.grads.clone()

    step()
    out1, g1 = step()
    given = xs[40:45]
    res = model.select_batch(xs[:40], 7, given=given, return_variance=True)
    again = model.select_batch(xs[:40], 7, given=given, return_variance=True)
    assert all(torch.equal(x, y) for x, y in zip(res, again))                          # the same call twice
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)                             # a training step does not see the call
    buf = io.BytesIO()
    torch.save({"model": copy.deepcopy(model)}, buf)
    buf.seek(0)
    snap = torch.load(buf, weights_only=False)["model"]
    assert callable(snap.select_batch)
    restored = snap.restore(mean_function=J.mean_fn(K))
    back = restored.select_batch(xs[:40], 7, given=given, return_variance=True)
    assert all(torch.equal(x, y) for x, y in zip(res, back))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_link_and_mean_do_not_enter(dtype):
    K, n = 3, 65
    plain, _, xs, _ = J.model_case(K, n, dtype)
    res = plain.select_batch(xs, 9, return_variance=True)
    other, _, _, _ = J.model_case(K, n, dtype, mean=True, link_function=lambda mu: torch.sigmoid(mu) / 2)
    assert all(torch.equal(x, y) for x, y in zip(res, other.select_batch(xs, 9, return_variance=True)))
