"""CPU tests of the Monte-Carlo predictive surface (csrc/predict_mc.h): the library exports its entry point, and the argument errors
are raised before any device call (a model cannot be built without a HIP device, so its methods are called unbound on a stub)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stub:
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    K, _K, _V, _link_function = 3, 3, 5, None


def test_library_exports_the_entry_point(hip_lib):
    from gdrf_amd import _lib
    assert hasattr(hip_lib, "gdrf_predict_mc")
    res, args = _lib.SIGNATURES["gdrf_predict_mc"]
    assert len(args) == 14       # ctx, X, n, Z, params, ws, mode, num_samples, seed, row_offset, eps, out, out_d, stream
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert re.search(r"\bint gdrf_predict_mc\(gdrf_ctx\* ctx, const void\* X_dev, int64_t n,", header)


def test_the_methods_exist_on_the_model_and_on_a_snapshot():
    from gdrf_amd.engine import Engine
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        for name in ("sample_topic_probs", "topic_probs_mc", "word_probs_mc", "predictive_perplexity"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Engine.predict_mc)


@pytest.mark.parametrize("num_samples", [0, -3])
def test_num_samples_below_one_is_a_value_error(num_samples):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    xs, ws = torch.rand(4, 2), torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="num_samples"):
        G.sample_topic_probs(Stub, xs, num_samples)
    with pytest.raises(ValueError, match="num_samples"):
        G.topic_probs_mc(Stub, xs, num_samples)
    with pytest.raises(ValueError, match="num_samples"):
        G.word_probs_mc(Stub, xs, num_samples)
    with pytest.raises(ValueError, match="num_samples"):
        G.predictive_perplexity(Stub, xs, ws, num_samples)


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 4, 3), (3, 3, 4), (2, 3), (2 * 3 * 4,)])
def test_an_eps_of_another_shape_is_a_value_error(shape):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="eps"):
        G.sample_topic_probs(Stub, torch.rand(4, 2), 2, eps=torch.zeros(shape))      # (S, K, n) = (2, 3, 4)


def test_sparse_counts_are_a_value_error():
    from gdrf_amd.data import to_csr
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import SparseMultinomialGDRF as G
    ws = to_csr(torch.ones(4, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="sparse"):
        G.predictive_perplexity(Stub, torch.rand(4, 2), ws, 8)
    with pytest.raises(ValueError, match="sparse"):
        Engine.predict_mc(Stub, torch.rand(4, 2), 2, 8, ws=ws, seed=1)
    with pytest.raises(ValueError, match="num_samples"):
        Engine.predict_mc(Stub, torch.rand(4, 2), 0, 0, seed=1)


def test_predictive_perplexity_with_a_custom_link_is_not_implemented():
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Linked(Stub):
        _link_function = staticmethod(lambda mu: torch.softmax(mu, -2))
    with pytest.raises(NotImplementedError, match="link_function"):
        G.predictive_perplexity(Linked, torch.rand(4, 2), torch.ones(4, 5, dtype=torch.int32), 8)
