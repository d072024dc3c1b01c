"""CPU tests of the credible-interval, exceedance and dominant-topic surface (csrc/predict_quant.h): the library exports its entry points,
header, ctypes table and engine constants agree, every argument error is raised before any device call (a model cannot be built without a
HIP device, so the methods are called unbound on a stub), and the float64 restatement of tests/_quant_ref.py is numpy's and torch's
"linear" quantile."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _quant_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTILE, EXCEED, DOMINANT = 0, 1, 2
XS = torch.rand(4, 2)


class Stub:
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    K, _K, V, _V, _link_function = 3, 3, 5, 5, None


class Linked(Stub):
    _link_function = staticmethod(lambda mu: torch.softmax(mu, -2))


def _G():
    from gdrf_amd.models import SparseMultinomialGDRF
    return SparseMultinomialGDRF


def _E():
    from gdrf_amd.engine import Engine
    return Engine


def test_library_header_table_and_engine_agree(hip_lib):
    from gdrf_amd import _lib, engine
    assert hasattr(hip_lib, "gdrf_predict_quant") and hasattr(hip_lib, "gdrf_quant_last_plan")
    _, args = _lib.SIGNATURES["gdrf_predict_quant"]
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    decl = re.search(r"\bint gdrf_predict_quant\(([^;]*)\);", header).group(1)
    assert len(args) == len(decl.split(",")) == 16
    assert len(_lib.SIGNATURES["gdrf_quant_last_plan"][1]) == 2
    assert int(re.search(r"#define GDRF_QUANT_MAX_SAMPLES (\d+)", header).group(1)) == engine.QUANT_MAX_SAMPLES == QR.MAX_SAMPLES == 1024
    assert int(re.search(r"#define GDRF_QUANT_MAX_LEVELS (\d+)", header).group(1)) == engine.QUANT_MAX_LEVELS == QR.MAX_LEVELS == 16
    assert re.search(r"enum \{ GDRF_QUANT_QUANTILE = 0, GDRF_QUANT_EXCEED = 1, GDRF_QUANT_DOMINANT = 2 \};", header)
    assert (engine.QUANT_QUANTILE, engine.QUANT_EXCEED, engine.QUANT_DOMINANT) == (QUANTILE, EXCEED, DOMINANT)


def test_the_methods_exist_on_the_model_and_on_a_snapshot():
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    for cls in (_G(), ModelSnapshot):
        for name in ("topic_probs_quantiles", "word_probs_quantiles", "exceedance", "dominant_topic_probs"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(_E().predict_quant) and callable(_E().last_quant_plan)


def _all_calls(num_samples=8, q=(0.5,), tau=(0.5,), eps=None):
    """every public way in, with the same sample count and eps"""
    G, E = _G(), _E()
    return [lambda: G.topic_probs_quantiles(Stub, XS, q, num_samples, eps=eps),
            lambda: G.word_probs_quantiles(Stub, XS, q, None, num_samples, eps=eps),
            lambda: G.exceedance(Stub, XS, tau, "topic", None, num_samples, eps=eps),
            lambda: G.exceedance(Stub, XS, tau, "word", [1, 2], num_samples, eps=eps),
            lambda: G.dominant_topic_probs(Stub, XS, num_samples, eps=eps),
            lambda: E.predict_quant(Stub, XS, QUANTILE, num_samples, levels=q, seed=1, eps=eps),
            lambda: E.predict_quant(Stub, XS, EXCEED, num_samples, levels=tau, seed=1, eps=eps),
            lambda: E.predict_quant(Stub, XS, DOMINANT, num_samples, seed=1, eps=eps)]


@pytest.mark.parametrize("num_samples", [0, -3])
def test_num_samples_below_one_is_a_value_error(num_samples):
    for call in _all_calls(num_samples):
        with pytest.raises(ValueError, match="num_samples"):
            call()


def test_the_sample_cap_binds_the_quantile_mode_only():
    G, E = _G(), _E()
    S = QR.MAX_SAMPLES + 1
    for call in (lambda: G.topic_probs_quantiles(Stub, XS, (0.5,), S), lambda: G.word_probs_quantiles(Stub, XS, (0.5,), None, S),
                 lambda: E.predict_quant(Stub, XS, QUANTILE, S, levels=(0.5,), seed=1)):
        with pytest.raises(ValueError, match="num_samples"):
            call()
    # the cap itself, and one more in the counter modes, pass the checks: the stub has nothing of what comes next
    for call in (lambda: G.topic_probs_quantiles(Stub, XS, (0.5,), QR.MAX_SAMPLES), lambda: G.exceedance(Stub, XS, 0.5, num_samples=S),
                 lambda: G.dominant_topic_probs(Stub, XS, S), lambda: E.predict_quant(Stub, XS, EXCEED, S, levels=(0.5,), seed=1)):
        with pytest.raises(AttributeError):
            call()
    for call in (lambda: G.exceedance(Stub, XS, 0.5, num_samples=65536), lambda: G.dominant_topic_probs(Stub, XS, 65536)):
        with pytest.raises(ValueError, match="num_samples"):
            call()


@pytest.mark.parametrize("levels", [(), [], tuple(i / 16 for i in range(17)), None])
def test_no_level_or_more_than_sixteen_is_a_value_error(levels):
    G, E = _G(), _E()
    for call in (lambda: G.topic_probs_quantiles(Stub, XS, levels, 8), lambda: G.word_probs_quantiles(Stub, XS, levels, None, 8),
                 lambda: G.exceedance(Stub, XS, levels, num_samples=8), lambda: E.predict_quant(Stub, XS, QUANTILE, 8, levels=levels, seed=1),
                 lambda: E.predict_quant(Stub, XS, EXCEED, 8, levels=levels, seed=1)):
        with pytest.raises(ValueError, match="level|threshold"):
            call()


def test_sixteen_levels_and_a_scalar_pass_the_checks():
    G = _G()
    for call in (lambda: G.topic_probs_quantiles(Stub, XS, tuple(i / 15 for i in range(16)), 8), lambda: G.topic_probs_quantiles(Stub, XS, 0.5, 8),
                 lambda: G.exceedance(Stub, XS, 0.25, num_samples=8), lambda: G.exceedance(Stub, XS, torch.tensor([0.0, 2.0, -1.0]), num_samples=8)):
        with pytest.raises(AttributeError):
            call()


@pytest.mark.parametrize("q", [-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf")])
def test_a_level_outside_the_unit_interval_is_a_value_error(q):
    G, E = _G(), _E()
    for call in (lambda: G.topic_probs_quantiles(Stub, XS, (0.5, q), 8), lambda: G.word_probs_quantiles(Stub, XS, (q,), None, 8),
                 lambda: E.predict_quant(Stub, XS, QUANTILE, 8, levels=(q,), seed=1)):
        with pytest.raises(ValueError, match="level"):
            call()


@pytest.mark.parametrize("tau", [float("nan"), float("inf"), -float("inf")])
def test_a_threshold_that_is_not_finite_is_a_value_error(tau):
    G, E = _G(), _E()
    for call in (lambda: G.exceedance(Stub, XS, (0.5, tau), num_samples=8), lambda: G.exceedance(Stub, XS, tau, "word", num_samples=8),
                 lambda: E.predict_quant(Stub, XS, EXCEED, 8, levels=(tau,), seed=1)):
        with pytest.raises(ValueError, match="threshold"):
            call()


@pytest.mark.parametrize("what", ["topics", "", None, 0, "WORD"])
def test_an_unknown_what_is_a_value_error(what):
    with pytest.raises(ValueError, match="what"):
        _G().exceedance(Stub, XS, 0.5, what, num_samples=8)


def test_words_with_topics_is_a_value_error():
    with pytest.raises(ValueError, match="words"):
        _G().exceedance(Stub, XS, 0.5, "topic", [0, 1], num_samples=8)
    with pytest.raises(ValueError, match="words"):
        _E().predict_quant(Stub, XS, DOMINANT, 8, words=torch.tensor([0], dtype=torch.int32), seed=1)


@pytest.mark.parametrize("words", [[5], [0, -1], [0, 1, 7, 2], torch.tensor([4, 5], dtype=torch.int32), [], [[0, 1]], [0.5], torch.tensor([1.0])])
def test_a_word_index_outside_the_vocabulary_is_a_value_error(words):
    G, E = _G(), _E()                       # V = 5
    for call in (lambda: G.word_probs_quantiles(Stub, XS, (0.5,), words, 8), lambda: G.exceedance(Stub, XS, 0.5, "word", words, 8),
                 lambda: E.predict_quant(Stub, XS, QUANTILE, 8, levels=(0.5,), words=words, seed=1),
                 lambda: E.predict_quant(Stub, XS, EXCEED, 8, levels=(0.5,), words=words, seed=1)):
        with pytest.raises(ValueError, match="word"):
            call()


def test_words_in_range_repeated_and_unordered_pass_the_checks():
    with pytest.raises(AttributeError):
        _G().word_probs_quantiles(Stub, XS, (0.5,), [4, 0, 0, 3], 8)


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 4, 3), (3, 3, 4), (2, 3), (2 * 3 * 4,)])
def test_an_eps_of_another_shape_is_a_value_error(shape):
    for call in _all_calls(2, eps=torch.zeros(shape)):          # (S, K, n) = (2, 3, 4)
        with pytest.raises(ValueError, match="eps"):
            call()


@pytest.mark.parametrize("mode", [-1, 3, "quantile", None])
def test_an_unknown_mode_is_a_value_error(mode):
    with pytest.raises(ValueError, match="mode"):
        _E().predict_quant(Stub, XS, mode, 8, levels=(0.5,), seed=1)


def test_a_custom_link_is_not_implemented_on_all_four_methods():
    G = _G()
    for call in (lambda: G.topic_probs_quantiles(Linked, XS), lambda: G.word_probs_quantiles(Linked, XS),
                 lambda: G.exceedance(Linked, XS, 0.5), lambda: G.dominant_topic_probs(Linked, XS)):
        with pytest.raises(NotImplementedError, match="link_function: the kernel fuses the softmax link"):
            call()


@pytest.mark.parametrize("S", [1, 2, 3, 7, 64, 1024])
def test_the_restatement_is_the_linear_quantile_of_numpy_and_torch(S):
    qs = (0.0, 0.025, 0.5, 1.0 / 3.0, 1.0)
    x = torch.rand(S, 5, 3, generator=torch.Generator().manual_seed(S), dtype=torch.float64)
    got = QR.quantiles_ref(x, qs)
    ends = QR.quantile_ends(x, qs)
    want_t = torch.quantile(x, torch.tensor(qs, dtype=torch.float64), dim=0, interpolation="linear")
    want_n = torch.from_numpy(np.quantile(x.numpy(), qs, axis=0))
    tol = 8 * 2.0 ** -53
    for name, want in (("torch", want_t), ("numpy", want_n)):
        err = float(((got - want).abs() / ends).max())
        print(f"S={S} {name}: {err:.2e}")
        assert err <= tol, (name, err)
    assert torch.equal(got[0], x.min(0).values) and torch.equal(got[-1], x.max(0).values)


def test_the_restatement_counts_strictly_and_breaks_ties_downwards():
    x = torch.tensor([0.25, 0.5, 0.5, 0.75], dtype=torch.float64).reshape(4, 1, 1)
    assert QR.exceed_counts_ref(x, (0.5, 0.25, 0.0, 0.75)).flatten().tolist() == [1, 3, 4, 0]
    th = torch.tensor([[[0.5, 0.5, 0.0]], [[0.2, 0.4, 0.4]], [[0.1, 0.2, 0.7]]], dtype=torch.float64)
    assert QR.dominant_counts_ref(th).tolist() == [[1, 1, 1]]
    assert QR.dominant_ref(th).sum().item() == 1.0
