"""CPU tests of the PSIS leave-one-out surface (csrc/predict_loo.h): the tail length against hand values, the float64 restatement of
tests/_loo_ref.py on tails laid on exact generalised-Pareto quantiles and on the degenerate rows, loo_from_pointwise and compare_pointwise
against numbers worked out by hand, every argument error before any device call (a model cannot be built without a HIP device, so its
methods are called on a stub), and the library's entry points, constants and names."""
import math
import os
import re

import pytest
import torch

from tests import _loo_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K, V, N = 32, 3, 5, 4
XS = torch.rand(N, 2)
WS = torch.ones(N, V, dtype=torch.int32)
TRUE_K = (-0.2, 0.0, 0.3, 0.7, 1.2)
# pareto_k of the restatement on the quantile-grid rows LR.gpd_tail_rows(1024, TRUE_K), as first computed (they are deterministic), beside
# the prior-shrunk true values (96 k + 5) / 106 = -0.1340, 0.0472, 0.3189, 0.6811, 1.1340
GRID_K_1024 = (-0.1123, 0.0627, 0.3237, 0.6714, 1.1061)


def stub(link=None):
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Stub:
        _K, _V, _link_function = K, V, link
        pointwise_loo = G.pointwise_loo
    Stub.K, Stub.V = K, V
    return Stub()


@pytest.mark.parametrize("num_samples,M", [(25, 5), (26, 6), (100, 20), (225, 45), (226, 46), (1024, 96)])
def test_the_tail_length_against_hand_values(num_samples, M):
    from gdrf_amd.engine import loo_tail_len
    assert loo_tail_len(num_samples) == LR.tail_len(num_samples) == M


def test_pareto_k_on_exact_gpd_tails_rises_with_the_true_k_and_lies_near_its_shrunk_value():
    for num_samples in (64, 256, 1024):
        k = LR.psis(LR.gpd_tail_rows(num_samples, TRUE_K))[1]
        print(num_samples, [round(float(v), 4) for v in k])
        assert bool((k[1:] > k[:-1]).all()), k
    M = LR.tail_len(1024)
    for got, true, seen in zip(k.tolist(), TRUE_K, GRID_K_1024):
        assert abs(got - (M * true + 5.0) / (M + 10.0)) <= 0.15 and abs(got - seen) < 5e-4, (got, true, seen)


def degenerate_rows(num_samples):
    """(S, 3): all values equal; all but four equal, the four below them; a tail whose lower quartile underflows"""
    a = torch.full((num_samples, 3), -5.0, dtype=torch.float64)
    a[:4, 1] = torch.tensor([-9.0, -8.0, -7.0, -6.0], dtype=torch.float64)
    a[:, 2] = -400.0 * torch.arange(num_samples, dtype=torch.float64)
    return a


def test_the_degenerate_rule():
    a = degenerate_rows(64)
    elpd, k, ess = LR.psis(a)
    assert bool(torch.isnan(k).all())
    assert abs(float(elpd[0]) + 5.0) < 1e-14 and abs(float(ess[0]) - 64.0) < 1e-11      # all equal: elpd_loo = a, ess = S
    # nothing is smoothed: the plain importance-sampling estimate, -log mean_s exp(-a_s)
    for c in (1, 2):
        plain = -(torch.logsumexp(-a[:, c], 0) - math.log(64))
        assert abs(float(elpd[c]) - float(plain)) < 1e-12 * abs(float(plain)), c
    assert abs(float(LR.psis(torch.zeros(25, 1, dtype=torch.float64))[0])) < 1e-15      # an empty row: 0


def test_a_small_relative_perturbation_of_a_moves_pareto_k_little():
    """what keeps float32 rounding of a_s out of the check of the PSIS arithmetic: 1e-7 relative on a of size 100 (1e-5 absolute) moves
    pareto_k by at most 2e-4"""
    g = torch.Generator().manual_seed(3)
    a = -100.0 + torch.randn(256, 50, generator=g, dtype=torch.float64)
    k0 = LR.psis(a)[1]
    k1 = LR.psis(a * (1.0 + 1e-7 * (2.0 * torch.rand(a.shape, generator=g, dtype=torch.float64) - 1.0)))[1]
    print(float((k1 - k0).abs().max()))
    assert float((k1 - k0).abs().max()) <= 2e-4


def test_loo_from_pointwise_against_numbers_worked_out_by_hand():
    """elpd_loo_n (-10.5, -20.1, -30.3), lpd (-10, -20, -30): the sum -60.9, p_loo 0.9, looic 121.8, se = sqrt(3 x 98.04) as WAIC's test
    works out; S = 64: k_threshold = 1 - 1 / log10(64) = 0.44635; pareto_k (0.2, NaN, 0.9): one bad, one not fitted."""
    from gdrf_amd.models import loo_from_pointwise
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)
    d = dict(elpd_loo=f64(-10.5, -20.1, -30.3), lpd=f64(-10.0, -20.0, -30.0), pareto_k=f64(0.2, float("nan"), 0.9), ess=f64(50.0, 64.0, 3.0))
    r = loo_from_pointwise(d, 64)
    assert set(r) == {"elpd_loo", "p_loo", "looic", "se", "pointwise", "pareto_k", "ess", "k_threshold", "n_bad_k", "n_not_fitted"}
    assert abs(float(r["elpd_loo"]) + 60.9) < 1e-13 and abs(float(r["p_loo"]) - 0.9) < 1e-13 and abs(float(r["looic"]) - 121.8) < 1e-13
    assert abs(float(r["se"]) - math.sqrt(294.12)) < 1e-12
    assert abs(r["k_threshold"] - (1.0 - 1.0 / math.log10(64))) < 1e-15 and abs(r["k_threshold"] - 0.44635) < 1e-5
    assert r["n_bad_k"] == 1 and r["n_not_fitted"] == 1 and type(r["n_bad_k"]) is int and type(r["n_not_fitted"]) is int
    assert torch.equal(r["pointwise"], d["elpd_loo"]) and torch.equal(r["ess"], d["ess"]) and r["elpd_loo"].dim() == 0 and r["se"].dim() == 0
    # S from the dict, then from log_lik; the threshold is capped at 0.7 (log10(S) > 10 / 3)
    assert loo_from_pointwise(dict(d, num_samples=1024))["k_threshold"] == 1.0 - 1.0 / math.log10(1024)
    assert loo_from_pointwise(dict(d, log_lik=torch.zeros(64, 3)))["k_threshold"] == r["k_threshold"]
    assert loo_from_pointwise(d, 4000)["k_threshold"] == 0.7 and loo_from_pointwise(d, 4000)["n_bad_k"] == 1
    with pytest.raises(ValueError, match="num_samples"):
        loo_from_pointwise(d)
    # one row: no standard error; the threshold itself is not above the threshold
    one = loo_from_pointwise(dict(elpd_loo=f64(-7.25), lpd=f64(-7.0), pareto_k=f64(0.7), ess=f64(9.0)), 4000)
    assert float(one["se"]) == 0.0 and float(one["elpd_loo"]) == -7.25 and float(one["p_loo"]) == 0.25 and float(one["looic"]) == 14.5
    assert one["n_bad_k"] == 0 and one["n_not_fitted"] == 0
    with pytest.raises(ValueError, match="maps"):
        loo_from_pointwise(dict(elpd_loo=torch.zeros(3), lpd=torch.zeros(2), pareto_k=torch.zeros(3), ess=torch.zeros(3)), 64)
    with pytest.raises(ValueError, match="maps"):
        loo_from_pointwise(dict(elpd_loo=torch.zeros(0), lpd=torch.zeros(0), pareto_k=torch.zeros(0), ess=torch.zeros(0)), 64)


def test_compare_pointwise_against_numbers_worked_out_by_hand():
    """a - b = (0.5, -0.1, 1.7): the sum 2.1, the mean 0.7, the deviations (-0.2, -0.8, 1.0), their squares sum to 1.68, the unbiased
    variance 0.84 and se_diff = sqrt(3 x 0.84) = sqrt(2.52)"""
    from gdrf_amd.models import compare_pointwise
    a, b = torch.tensor([-10.5, -20.1, -30.3], dtype=torch.float64), torch.tensor([-11.0, -20.0, -32.0], dtype=torch.float64)
    r = compare_pointwise(a, b)
    assert set(r) == {"elpd_diff", "se_diff"}
    assert abs(float(r["elpd_diff"]) - 2.1) < 1e-13 and abs(float(r["se_diff"]) - math.sqrt(2.52)) < 1e-13
    back = compare_pointwise(b, a)
    assert float(back["elpd_diff"]) == -float(r["elpd_diff"]) and abs(float(back["se_diff"]) - float(r["se_diff"])) < 1e-15
    one = compare_pointwise(a[:1], b[:1].float())
    assert float(one["elpd_diff"]) == 0.5 and float(one["se_diff"]) == 0.0 and one["elpd_diff"].dtype == torch.float64
    for x, y in ((a, b[:2]), (a[:0], b[:0]), (a[None], b[None])):
        with pytest.raises(ValueError, match="pointwise"):
            compare_pointwise(x, y)


def test_library_exports_the_entry_points_and_the_constants_agree(hip_lib):
    from gdrf_amd import _lib, engine
    for name, nargs in (("gdrf_predict_loo", 17), ("gdrf_psis_rows", 7), ("gdrf_loo_last_plan", 2)):
        assert hasattr(hip_lib, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert re.search(r"\bint gdrf_predict_loo\(gdrf_ctx\* ctx, const void\* X_dev, int64_t n,", header)
    assert re.search(r"\bint gdrf_psis_rows\(gdrf_ctx\* ctx, const double\* log_lik_dev, int num_samples, int tail_len, int64_t n,", header)
    kernel = open(os.path.join(ROOT, "gdrf_amd", "csrc", "predict_loo.h")).read()
    for text in (header, kernel):
        assert int(re.search(r"#define GDRF_LOO_MAX_SAMPLES (\d+)", text).group(1)) == engine.LOO_MAX_SAMPLES == LR.MAX_SAMPLES == 1024
        assert int(re.search(r"#define GDRF_LOO_MIN_SAMPLES (\d+)", text).group(1)) == engine.LOO_MIN_SAMPLES == LR.MIN_SAMPLES == 25
    assert int(re.search(r"constexpr int PSIS_LG = (\d+);", kernel).group(1)) == LR.PSIS_LG
    assert engine.LOO_NAMES == LR.NAMES == ("elpd_loo", "pareto_k", "ess", "lpd", "total", "log_coef")


def test_the_methods_exist_on_the_model_and_the_snapshot_list_is_unchanged():
    from gdrf_amd import models
    from gdrf_amd.engine import Engine
    from gdrf_amd.models.sparse_gdrf import SNAPSHOT_METHODS, SparseMultinomialGDRF
    for name in ("pointwise_loo", "loo", "psis"):
        assert callable(getattr(SparseMultinomialGDRF, name)) and name not in SNAPSHOT_METHODS
        assert "snap.restore()" in getattr(SparseMultinomialGDRF, name).__doc__
    assert len(SNAPSHOT_METHODS) == 27
    for name in ("predict_loo", "psis_rows", "last_loo_plan"):
        assert callable(getattr(Engine, name))
    assert callable(models.loo_from_pointwise) and callable(models.compare_pointwise)
    assert {"loo_from_pointwise", "compare_pointwise", "waic_from_pointwise"} <= set(models.__all__)


def every_surface(num_samples, ws=WS, eps=None, match=None):
    """check_loo_args and everything above it raise the same ValueError"""
    from gdrf_amd.engine import Engine, check_loo_args
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match=match):
        check_loo_args(num_samples, K, V, N, ws, eps)
    with pytest.raises(ValueError, match=match):
        Engine.predict_loo(stub(), XS, ws, num_samples, seed=1, eps=eps)
    with pytest.raises(ValueError, match=match):
        G.pointwise_loo(stub(), XS, ws, num_samples, eps=eps)
    if eps is None:
        with pytest.raises(ValueError, match=match):
            G.loo(stub(), XS, ws, num_samples)


@pytest.mark.parametrize("num_samples", [True, False, 32.5, "many", None, float("nan"), float("inf")])
def test_a_num_samples_that_is_no_integer_is_a_value_error(num_samples):
    every_surface(num_samples, match="num_samples must be an integer")


@pytest.mark.parametrize("num_samples", [0, -3, 1, 24, 1025, 65535, 1e6])
def test_a_num_samples_out_of_range_is_a_value_error(num_samples):
    every_surface(num_samples, match="num_samples must be in 25 .. 1024")


@pytest.mark.parametrize("num_samples", [25, 256, 1024, 64.0])
def test_a_num_samples_in_range_comes_back_as_an_int(num_samples):
    from gdrf_amd.engine import check_loo_args
    got = check_loo_args(num_samples, K, V, N, WS)
    assert got == int(num_samples) and type(got) is int


@pytest.mark.parametrize("shape", [(32, 3, 5), (32, 4, 4), (31, 3, 4), (32, 3), (32 * 3 * 4,)])
def test_an_eps_of_another_shape_is_a_value_error(shape):
    every_surface(S, eps=torch.zeros(shape), match="eps must have shape")             # (S, K, n) = (32, 3, 4)


@pytest.mark.parametrize("ws", [None, torch.ones(N, V + 1, dtype=torch.int32), torch.ones(N + 1, V, dtype=torch.int32),
                                torch.ones(N * V, dtype=torch.int32), [[1] * V] * N,
                                torch.ones(N, V + 1, dtype=torch.int32).to_sparse_csr()], ids=["none", "V", "n", "flat", "list", "csr_V"])
def test_counts_of_another_shape_are_a_value_error(ws):
    every_surface(S, ws=ws, match="ws must be counts of shape")


def test_arguments_of_the_right_shape_pass_and_no_row_is_refused():
    from gdrf_amd.engine import check_loo_args
    assert check_loo_args(S, K, V, N, WS, torch.zeros(S, K, N)) == S and check_loo_args(S, K, V, N, WS.to_sparse_csr()) == S
    with pytest.raises(ValueError, match="at least one row"):
        check_loo_args(S, K, V, 0, torch.ones(0, V, dtype=torch.int32))


@pytest.mark.parametrize("log_lik,match", [(torch.zeros(24, 3), "25 .. 1024"), (torch.zeros(1025, 3), "25 .. 1024"), (torch.zeros(32), "log_lik must be"),
                                           (torch.zeros(32, 0), "log_lik must be"), (torch.zeros(2, 32, 3), "log_lik must be"),
                                           ([[0.0] * 3] * 32, "log_lik must be")], ids=["S24", "S1025", "flat", "no_rows", "3d", "list"])
def test_the_stage_refuses_a_matrix_of_another_shape(log_lik, match):
    from gdrf_amd.engine import Engine, check_psis_args
    with pytest.raises(ValueError, match=match):
        check_psis_args(log_lik)
    with pytest.raises(ValueError, match=match):
        Engine.psis_rows(stub(), log_lik)
    assert check_psis_args(torch.zeros(25, 1)) == (25, 1) and check_psis_args(torch.zeros(1024, 7)) == (1024, 7)


def test_a_custom_link_is_not_implemented_and_the_message_names_psis():
    from gdrf_amd.models import SparseMultinomialGDRF as G
    linked = stub(link=staticmethod(lambda mu: torch.softmax(mu, -2)))
    for call in (lambda: G.pointwise_loo(linked, XS, WS, S), lambda: G.loo(linked, XS, WS, S)):
        with pytest.raises(NotImplementedError, match="link_function.*psis"):
            call()


def test_valid_arguments_reach_the_device_layer():
    """The checks pass: the stub has no _prepare_inputs, which is the next thing the method touches"""
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(AttributeError, match="_prepare_inputs"):
        G.pointwise_loo(stub(), XS, WS, S)
