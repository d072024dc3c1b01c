"""CPU tests of the per-row predictive-density and WAIC surface (csrc/predict_score.h): the library exports its entry point, the argument
errors are raised before any device call (a model cannot be built without a HIP device, so its methods are called on a stub), and the
WAIC arithmetic against numbers worked out by hand."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lpd", "mean_log_lik", "var_log_lik", "total", "log_coef")
S, K, V, N = 2, 3, 5, 4
XS = torch.rand(N, 2)
WS = torch.ones(N, V, dtype=torch.int32)


def stub(link=None):
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Stub:
        _K, _V, _link_function = K, V, link
        pointwise_log_likelihood = G.pointwise_log_likelihood
    Stub.K, Stub.V = K, V
    return Stub()


def test_library_exports_the_entry_point_and_the_constants_agree(hip_lib):
    from gdrf_amd import _lib, engine
    assert hasattr(hip_lib, "gdrf_predict_score")
    res, args = _lib.SIGNATURES["gdrf_predict_score"]
    assert len(args) == 15      # ctx, X, n, Z, params, ws, crow, col, val, num_samples, seed, row_offset, eps, out, stream
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert re.search(r"\bint gdrf_predict_score\(gdrf_ctx\* ctx, const void\* X_dev, int64_t n,", header)
    assert int(re.search(r"#define GDRF_SCORE_V_CHUNK (\d+)", header).group(1)) == engine.SCORE_V_CHUNK == 128
    assert int(re.search(r"#define GDRF_SCORE_S_TILE (\d+)", header).group(1)) == engine.SCORE_S_TILE == 64
    kernel = open(os.path.join(ROOT, "gdrf_amd", "csrc", "predict_score.h")).read()
    assert int(re.search(r"#define GDRF_SCORE_V_CHUNK (\d+)", kernel).group(1)) == engine.SCORE_V_CHUNK
    assert int(re.search(r"#define GDRF_SCORE_S_TILE (\d+)", kernel).group(1)) == engine.SCORE_S_TILE
    assert engine.SCORE_NAMES == NAMES


def test_the_methods_exist_on_the_model_and_on_a_snapshot():
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import waic_from_pointwise
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        for name in ("pointwise_log_likelihood", "waic", "row_perplexity"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Engine.predict_score) and callable(waic_from_pointwise)


def test_a_snapshot_passes_every_argument_through():
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    calls = []

    class Model:
        def pointwise_log_likelihood(self, xs, ws, num_samples=64, seed=None, eps=None, normalized=False):
            calls.append(("pointwise", xs, ws, num_samples, seed, eps, normalized))
            return "p"

        def waic(self, xs, ws, num_samples=64, seed=None, normalized=False):
            calls.append(("waic", xs, ws, num_samples, seed, normalized))
            return "w"

        def row_perplexity(self, xs, ws, num_samples=64, seed=None):
            calls.append(("row", xs, ws, num_samples, seed))
            return "r"

    class Snap:
        def restore(self):
            return Model()
    assert ModelSnapshot.pointwise_log_likelihood(Snap(), XS, WS, 7, seed=3, eps="e", normalized=True) == "p"
    assert ModelSnapshot.waic(Snap(), XS, WS, 8, seed=4, normalized=True) == "w"
    assert ModelSnapshot.row_perplexity(Snap(), XS, WS, 9, seed=5) == "r"
    assert calls == [("pointwise", XS, WS, 7, 3, "e", True), ("waic", XS, WS, 8, 4, True), ("row", XS, WS, 9, 5)]
    # the defaults are the model's
    ModelSnapshot.pointwise_log_likelihood(Snap(), XS, WS)
    ModelSnapshot.waic(Snap(), XS, WS)
    ModelSnapshot.row_perplexity(Snap(), XS, WS)
    assert calls[3:] == [("pointwise", XS, WS, 64, None, None, False), ("waic", XS, WS, 64, None, False), ("row", XS, WS, 64, None)]


def every_surface(num_samples, ws=WS, eps=None, match=None):
    """check_score_args and everything above it raise the same ValueError"""
    from gdrf_amd.engine import Engine, check_score_args
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match=match):
        check_score_args(num_samples, K, V, N, ws, eps)
    with pytest.raises(ValueError, match=match):
        Engine.predict_score(stub(), XS, ws, num_samples, seed=1, eps=eps)
    with pytest.raises(ValueError, match=match):
        G.pointwise_log_likelihood(stub(), XS, ws, num_samples, eps=eps)
    if eps is None:
        with pytest.raises(ValueError, match=match):
            G.waic(stub(), XS, ws, num_samples)
        with pytest.raises(ValueError, match=match):
            G.row_perplexity(stub(), XS, ws, num_samples)


@pytest.mark.parametrize("num_samples", [True, False, 2.5, "many", None, float("nan"), float("inf")])
def test_a_num_samples_that_is_no_integer_is_a_value_error(num_samples):
    every_surface(num_samples, match="num_samples must be an integer")


@pytest.mark.parametrize("num_samples", [0, -3, 65536, 1e6])
def test_a_num_samples_out_of_range_is_a_value_error(num_samples):
    every_surface(num_samples, match="num_samples must be in 1 .. 65535")


@pytest.mark.parametrize("num_samples", [1, 64, 65535, 2.0])
def test_a_num_samples_in_range_comes_back_as_an_int(num_samples):
    from gdrf_amd.engine import check_score_args
    got = check_score_args(num_samples, K, V, N, WS)
    assert got == int(num_samples) and type(got) is int


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 4, 4), (3, 3, 4), (2, 3), (2 * 3 * 4,)])
def test_an_eps_of_another_shape_is_a_value_error(shape):
    every_surface(S, eps=torch.zeros(shape), match="eps must have shape")             # (S, K, n) = (2, 3, 4)


def test_an_eps_of_the_right_shape_passes():
    from gdrf_amd.engine import check_score_args
    assert check_score_args(S, K, V, N, WS, torch.zeros(S, K, N)) == S


@pytest.mark.parametrize("ws", [None, torch.ones(N, V + 1, dtype=torch.int32), torch.ones(N + 1, V, dtype=torch.int32),
                                torch.ones(N * V, dtype=torch.int32), [[1] * V] * N,
                                torch.ones(N, V + 1, dtype=torch.int32).to_sparse_csr()], ids=["none", "V", "n", "flat", "list", "csr_V"])
def test_counts_of_another_shape_are_a_value_error(ws):
    every_surface(S, ws=ws, match="ws must be counts of shape")


def test_counts_of_the_right_shape_pass_dense_and_csr():
    from gdrf_amd.engine import check_score_args
    assert check_score_args(S, K, V, N, WS) == S
    assert check_score_args(S, K, V, N, WS.to_sparse_csr()) == S
    with pytest.raises(ValueError, match="at least one row"):
        check_score_args(S, K, V, 0, torch.ones(0, V, dtype=torch.int32))


def test_a_custom_link_is_not_implemented():
    from gdrf_amd.models import SparseMultinomialGDRF as G
    linked = stub(link=staticmethod(lambda mu: torch.softmax(mu, -2)))
    for call in (lambda: G.pointwise_log_likelihood(linked, XS, WS, 8), lambda: G.waic(linked, XS, WS, 8), lambda: G.row_perplexity(linked, XS, WS, 8)):
        with pytest.raises(NotImplementedError, match="link_function"):
            call()


def test_valid_arguments_reach_the_device_layer():
    """The checks pass: the stub has no _prepare_inputs, which is the next thing the method touches"""
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(AttributeError, match="_prepare_inputs"):
        G.pointwise_log_likelihood(stub(), XS, WS, 8)


def test_waic_from_pointwise_against_numbers_worked_out_by_hand():
    """lpd (-10, -20, -30), var (0.5, 0.1, 0.3): elpd_n = (-10.5, -20.1, -30.3), their sum -60.9, p_waic 0.9, waic 121.8; the mean of
    elpd_n is -20.3, the deviations (9.8, 0.2, -10.0), their squares sum to 196.08, the unbiased variance is 98.04 and
    se = sqrt(3 x 98.04) = sqrt(294.12); one row (0.5) is above 0.4."""
    from gdrf_amd.models import waic_from_pointwise
    d = dict(lpd=torch.tensor([-10.0, -20.0, -30.0], dtype=torch.float64), var_log_lik=torch.tensor([0.5, 0.1, 0.3], dtype=torch.float64))
    w = waic_from_pointwise(d)
    assert set(w) == {"elpd_waic", "p_waic", "waic", "se", "pointwise", "n_high_variance"}
    assert torch.allclose(w["pointwise"], torch.tensor([-10.5, -20.1, -30.3], dtype=torch.float64), rtol=0, atol=1e-14)
    assert abs(float(w["elpd_waic"]) + 60.9) < 1e-13 and abs(float(w["p_waic"]) - 0.9) < 1e-15 and abs(float(w["waic"]) - 121.8) < 1e-13
    assert abs(float(w["se"]) - math.sqrt(294.12)) < 1e-12
    assert w["n_high_variance"] == 1 and type(w["n_high_variance"]) is int
    assert w["pointwise"].dtype == torch.float64 and w["elpd_waic"].dim() == 0 and w["se"].dim() == 0
    # 0.4 itself is not above 0.4; float32 maps are widened
    w = waic_from_pointwise(dict(lpd=torch.tensor([-1.0, -2.0]), var_log_lik=torch.tensor([0.4, 0.5], dtype=torch.float64)))
    assert w["n_high_variance"] == 1 and w["pointwise"].dtype == torch.float64


def test_waic_of_one_draw_has_no_penalty_and_of_one_row_no_standard_error():
    from gdrf_amd.models import waic_from_pointwise
    lpd = torch.tensor([-3.0, -5.0, -4.0], dtype=torch.float64)
    w = waic_from_pointwise(dict(lpd=lpd, var_log_lik=torch.zeros(3, dtype=torch.float64)))             # S = 1: var_log_lik is 0
    assert float(w["p_waic"]) == 0.0 and torch.equal(w["pointwise"], lpd) and float(w["elpd_waic"]) == -12.0 and float(w["waic"]) == 24.0
    assert abs(float(w["se"]) - math.sqrt(3.0 * 1.0)) < 1e-15 and w["n_high_variance"] == 0           # the variance of (-3, -5, -4) is 1
    w = waic_from_pointwise(dict(lpd=torch.tensor([-7.0], dtype=torch.float64), var_log_lik=torch.tensor([0.25], dtype=torch.float64)))
    assert float(w["se"]) == 0.0 and float(w["elpd_waic"]) == -7.25 and float(w["p_waic"]) == 0.25 and float(w["waic"]) == 14.5
    with pytest.raises(ValueError, match="maps"):
        waic_from_pointwise(dict(lpd=torch.zeros(3), var_log_lik=torch.zeros(2)))
    with pytest.raises(ValueError, match="maps"):
        waic_from_pointwise(dict(lpd=torch.zeros(0), var_log_lik=torch.zeros(0)))
