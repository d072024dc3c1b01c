"""CPU tests of the choice of inducing points (csrc/select_inducing.h): the two forms of the float64 restatement (tests/_inducing_ref.py)
agree, the library exports its entry point, the methods exist, every argument error is raised before any device call (a model cannot be
built without a HIP device, so its methods are called unbound on a stub and the constructor is called with arguments that fail first), the
thinning rule, and the margins the GPU tests (tests/test_gpu_select_inducing.py) rely on, so that a bad seed is caught without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _inducing_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stub:
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    K, _K, M, _link_function = 3, 3, 7, None


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_loop_and_the_dense_solve_agree_after_every_pick(kind):
    """d and the trace of the loop against diag(K_nn - K_nP K_PP^-1 K_Pn) by a dense solve on the picks so far, with 3 given rows first.
    The bound: the loop's smallest pivot is asserted to stay above 1e-4 of the variance, so cond(K_PP) <= |P| var / 1e-4 var = 2.3e5 and
    the dense solve carries about cond eps = 5e-11 of the variance; 1e-9 leaves a factor of twenty."""
    D = 1 if kind == "periodic" else 2
    kern = R.Kern(kind, D, ls=0.15)
    X, given = R.uniform_rows(5, 120, D), R.uniform_rows(6, 3, D)
    count = 6 if kind == "periodic" else 20                # a one-dimensional periodic kernel at ls 0.8 has few directions to explain
    run = R.greedy(kern, X, count, given=given)
    assert run["rank"] == 3 + count and run["pivots"].min() > 1e-4 * kern.variance
    for t in range(3 + count):
        P = np.concatenate([given[:min(t + 1, 3)], X[run["picks"][:max(t + 1 - 3, 0)]]])
        d = R.nystrom_residual(kern, X, P)
        part = R.greedy(kern, X, max(t + 1 - 3, 0), given=given[:min(t + 1, 3)], forced=run["picks"])
        assert np.abs(part["d"] - d).max() < 1e-9 * kern.variance, (t, np.abs(part["d"] - d).max())
        assert abs(run["trace"][t] - d.sum()) < 120 * 1e-9 * kern.variance, t
    assert np.all(np.diff(run["trace"]) <= 0) and np.all(np.diff(run["pivots"][3:]) <= 1e-12 * kern.variance)
    assert len(set(run["picks"])) == count


def test_the_restatement_is_degenerate_where_it_should_be():
    """duplicates: 40 places three times each, 50 picks: rank 40, the first 40 picks the first copies, the last 10 pivots at most the floor"""
    kern = R.Kern("rbf", 2, ls=0.2)
    floor = 50 * np.finfo(np.float64).eps * kern.variance
    run = R.greedy(kern, R.duplicated_rows(), 50, floor=floor)
    assert run["rank"] == 40 and sorted(run["picks"][:40]) == list(range(40))
    assert run["pivots"][:40].min() > 1e3 * floor and np.abs(run["pivots"][40:]).max() <= floor
    # a given row twice: the second is a degenerate pick and changes nothing
    X, g = R.uniform_rows(1, 30, 2), R.uniform_rows(2, 1, 2)
    once, twice = R.greedy(kern, X, 4, given=g, floor=floor), R.greedy(kern, X, 4, given=np.concatenate([g, g]), floor=floor)
    assert twice["rank"] == once["rank"] == 5 and twice["picks"] == once["picks"]
    assert np.abs(twice["d"] - once["d"]).max() <= floor


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: f"seed{c[0]}-{c[4]}")
def test_margins_of_the_exact_pick_cases(case):
    """what test_gpu_select_inducing.py's exact-pick test asserts again on the GPU machine: at every step the best d leads the runner-up by
    at least EXACT_GAP of the variance, far above float64 rounding of a history of M products (M eps = 2e-14)"""
    seed, n, D, M, kind, ls = case
    kern = R.Kern(kind, D, ls=ls)
    run = R.greedy(kern, R.uniform_rows(seed, n, D), M)
    print(f"seed {seed} {kind}: smallest gap {run['gap'] / kern.variance:.3e} of the variance")
    assert run["gap"] >= R.EXACT_GAP * kern.variance and run["rank"] == M


def test_mesh_against_greedy_on_a_track():
    """the reason for all this: 36 greedy picks on a spiral track leave a tenth of what the 6 x 6 mesh leaves"""
    kern = R.Kern("rbf", 2, ls=0.1)
    X = R.spiral_track()
    assert X.shape == (600, 2) and X.min() >= 0 and X.max() <= 1
    mesh = R.greedy(kern, X, 0, given=R.mesh(6))
    run = R.greedy(kern, X, 36)
    scale = 600 * kern.variance
    print(f"residual trace / (n var): mesh {mesh['trace'][-1] / scale:.3f}, greedy {run['trace'][-1] / scale:.3f}")
    assert abs(mesh["trace"][-1] - R.nystrom_residual(kern, X, R.mesh(6)).sum()) < 1e-9 * scale
    assert abs(run["trace"][-1] - R.nystrom_residual(kern, X, X[run["picks"]]).sum()) < 1e-9 * scale
    assert abs(mesh["trace"][-1] / scale - 0.330) < 2e-3 and abs(run["trace"][-1] / scale - 0.034) < 2e-3
    assert run["trace"][-1] < 0.5 * mesh["trace"][-1]


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point(hip_lib):
    from gdrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert hasattr(hip_lib, "gdrf_select_inducing")
    assert len(_lib.SIGNATURES["gdrf_select_inducing"][1]) == 14
    decl = re.search(r"\bint gdrf_select_inducing\(gdrf_ctx\* ctx,([^;]*)\);", header)
    assert decl and decl.group(1).count(",") + 2 == 14           # the header's argument count
    assert "#define GDRF_INDUCING_MAX_PICKS 1024" in header


def test_the_methods_exist_on_the_model_the_snapshot_and_the_engine():
    from gdrf_amd.engine import INDUCING_MAX_PICKS, Engine, check_inducing_args
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    assert callable(Engine.select_inducing)
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        assert callable(getattr(cls, "choose_inducing_points")), cls
    snap, model = vars(ModelSnapshot)["choose_inducing_points"], vars(SparseMultinomialGDRF)["choose_inducing_points"]
    assert snap is not model and snap.__doc__ is model.__doc__ and snap.__qualname__ == "ModelSnapshot.choose_inducing_points"

    class Restored:
        def choose_inducing_points(self, *a, **kw):
            return a, kw

    class Snap:
        def restore(self):
            return Restored()
    assert ModelSnapshot.choose_inducing_points(Snap(), 1, count=2) == ((1,), dict(count=2))     # forwarded to restore(), as the others are
    assert INDUCING_MAX_PICKS == 1024 and callable(check_inducing_args)
    assert "same" in SparseMultinomialGDRF.__init__.__doc__ and "rank" in SparseMultinomialGDRF.__init__.__doc__


def test_check_inducing_args_accepts_what_it_should():
    from gdrf_amd.engine import INDUCING_MAX_PICKS, check_inducing_args
    assert check_inducing_args(1, 0.0, 1) == (1, 0.0, 0)
    assert check_inducing_args(4, 1e-3, 4) == (4, 1e-3, 0)
    c, f, G = check_inducing_args(3.0, 2, 10)
    assert (c, f, G) == (3, 2.0, 0) and isinstance(c, int) and isinstance(f, float)
    assert check_inducing_args(3, None, 10) == (3, None, 0)                          # the model fills in its own floor
    assert check_inducing_args(0, 0.0, 10, given=torch.zeros(5, 2), dims=2) == (0, 0.0, 5)       # scoring an existing set
    assert check_inducing_args(3, 0.0, 10, given=torch.zeros(0, 2), dims=2) == (3, 0.0, 0)
    assert check_inducing_args(INDUCING_MAX_PICKS, 0.0, 1100) == (INDUCING_MAX_PICKS, 0.0, 0)
    assert check_inducing_args(INDUCING_MAX_PICKS - 5, 0.0, 1100, given=torch.zeros(5, 2), dims=2)[2] == 5
    assert check_inducing_args(2, 0.0, 7, given=torch.zeros(4), dims=1)[2] == 4


def raises_everywhere(match, xs, count, floor=0.0, given=None):
    from gdrf_amd.engine import Engine, check_inducing_args
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match=match):
        check_inducing_args(count, floor, int(xs.shape[0]), given, int(xs.shape[1]))
    with pytest.raises(ValueError, match=match):
        Engine.select_inducing(Stub, xs, count, given=given, floor=floor)
    if floor == 0.0:                                             # the model computes its own floor
        with pytest.raises(ValueError, match=match):
            G.choose_inducing_points(Stub, xs, count, given=given)


@pytest.mark.parametrize("count", [-1, 2.5, True, 5, "3"])
def test_count_must_be_an_integer_between_zero_and_the_rows(count):
    raises_everywhere("count", torch.rand(4, 2), count)


def test_no_picks_and_no_given_rows_is_an_error():
    raises_everywhere("at least 1", torch.rand(4, 2), 0)
    raises_everywhere("at least 1", torch.rand(4, 2), 0, given=torch.zeros(0, 2))


def test_no_rows_is_an_error():
    raises_everywhere("at least one row", torch.rand(0, 2), 1)


def test_the_given_rows_and_the_picks_share_the_cap():
    from gdrf_amd.engine import INDUCING_MAX_PICKS
    xs = torch.rand(INDUCING_MAX_PICKS + 44, 2)
    raises_everywhere("INDUCING_MAX_PICKS", xs, INDUCING_MAX_PICKS + 1)
    raises_everywhere("INDUCING_MAX_PICKS", xs, INDUCING_MAX_PICKS - 4, given=torch.rand(5, 2))


@pytest.mark.parametrize("floor", [-1.0, -1e-300, float("nan"), float("inf"), -float("inf"), True])
def test_floor_must_be_finite_and_not_negative(floor):
    raises_everywhere("floor", torch.rand(4, 2), 2, floor=floor)


@pytest.mark.parametrize("shape", [(3, 1), (3, 3), (6,), (1, 3, 2)])
def test_a_given_with_other_columns_is_a_value_error(shape):
    raises_everywhere("given", torch.rand(4, 2), 2, given=torch.zeros(shape))


def test_the_engine_needs_a_floor():
    from gdrf_amd.engine import Engine
    with pytest.raises(ValueError, match="floor"):
        Engine.select_inducing(Stub, torch.rand(4, 2), 2, floor=None)


def test_the_thinning_rule():
    from gdrf_amd.engine import thin_rows
    assert thin_rows(10, 10) is None and thin_rows(3, 131072) is None and thin_rows(1, 1) is None
    for n, c in ((11, 10), (1000, 7), (131073, 131072), (10 ** 6, 131072), (5, 1)):
        t = thin_rows(n, c)
        assert t.dtype == torch.int64 and t.tolist() == [i * n // c for i in range(c)]
        assert int(t[0]) == 0 and int(t[-1]) < n and bool((t[1:] > t[:-1]).all())
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_candidates"):
            thin_rows(10, bad)
    # more rows than max_candidates: the count is checked against the thinned rows, before the device
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="count"):
        G.choose_inducing_points(Stub, torch.rand(100, 2), 11, max_candidates=10)
    with pytest.raises(ValueError, match="max_candidates"):
        G.choose_inducing_points(Stub, torch.rand(100, 2), 5, max_candidates=0)


# ---- the constructor: these fail before a device is touched (on this machine building an engine would raise GdrfHipError instead) -------------
def build(**kw):
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    args = dict(num_observation_categories=5, num_topic_categories=2, world=[(0.0, 1.0)] * 2,
                kernel=RBF(input_dim=2, lengthscale=torch.tensor(0.3), variance=torch.tensor(25.0)), dirichlet_param=0.01, n_points=[3, 3],
                fixed_inducing_points=True, dtype=torch.float64)
    args.update(kw)
    return SparseMultinomialGDRF(**args)


def test_greedy_needs_candidates():
    with pytest.raises(ValueError, match="inducing_candidates"):
        build(inducing_init="greedy")


def test_greedy_candidates_are_checked_before_the_device():
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        build(inducing_init="greedy", inducing_candidates=torch.rand(20, 3))
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        build(inducing_init="greedy", xs=torch.rand(20))
    with pytest.raises(ValueError, match="count"):               # fewer candidates than M = 9
        build(inducing_init="greedy", inducing_candidates=torch.rand(8, 2))
    with pytest.raises(ValueError, match="INDUCING_MAX_PICKS"):
        build(inducing_init="greedy", inducing_candidates=torch.rand(2000, 2), n_points=[40, 40])


def test_an_unknown_inducing_init_keeps_its_message():
    with pytest.raises(ValueError, match="inducing_init argument kmeans not valid. Only 'random' and 'grid' are currently supported") as e:
        build(inducing_init="kmeans")
    assert "greedy" in str(e.value)


def test_train_takes_the_method():
    import inspect
    from gdrf_amd.train import train
    assert "greedy" in train.__doc__ and "inducing_initialization_method" in inspect.signature(train).parameters
