"""CPU tests of the entropy and information-gain surface (csrc/predict_info.h): the library exports its entry point, and the argument
errors are raised before any device call (a model cannot be built without a HIP device, so its methods are called unbound on a stub)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("topic_entropy", "topic_expected_entropy", "topic_information", "word_entropy", "word_expected_entropy", "word_information")


class Stub:
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs, information) is an AttributeError"""
    K, _K, _V, _link_function = 3, 3, 5, None


def test_library_exports_the_entry_point(hip_lib):
    from gdrf_amd import _lib, engine
    assert hasattr(hip_lib, "gdrf_predict_info")
    res, args = _lib.SIGNATURES["gdrf_predict_info"]
    assert len(args) == 11       # ctx, X, n, Z, params, num_samples, seed, row_offset, eps, out, stream
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert re.search(r"\bint gdrf_predict_info\(gdrf_ctx\* ctx, const void\* X_dev, int64_t n,", header)
    assert int(re.search(r"#define GDRF_INFO_V_CHUNK (\d+)", header).group(1)) == engine.INFO_V_CHUNK
    assert engine.INFO_NAMES == NAMES


def test_the_methods_exist_on_the_model_and_on_a_snapshot():
    from gdrf_amd.engine import Engine
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        for name in ("information", "most_informative"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Engine.predict_info)


@pytest.mark.parametrize("num_samples", [0, -3])
def test_num_samples_below_one_is_a_value_error(num_samples):
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="num_samples"):
        G.information(Stub, torch.rand(4, 2), num_samples)
    with pytest.raises(ValueError, match="num_samples"):
        Engine.predict_info(Stub, torch.rand(4, 2), num_samples, seed=1)


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 4, 3), (3, 3, 4), (2, 3), (2 * 3 * 4,)])
def test_an_eps_of_another_shape_is_a_value_error(shape):
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="eps"):
        G.information(Stub, torch.rand(4, 2), 2, eps=torch.zeros(shape))           # (S, K, n) = (2, 3, 4)
    with pytest.raises(ValueError, match="eps"):
        Engine.predict_info(Stub, torch.rand(4, 2), 2, eps=torch.zeros(shape))


@pytest.mark.parametrize("criterion", ["information", "word_info", "", None, 5])
def test_an_unknown_criterion_is_a_value_error(criterion):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="criterion"):
        G.most_informative(Stub, torch.rand(4, 2), 2, criterion)


@pytest.mark.parametrize("count", [0, -1, 5, 2.5, True])
def test_a_count_out_of_range_is_a_value_error(count):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    for criterion in NAMES:
        with pytest.raises(ValueError, match="count"):
            G.most_informative(Stub, torch.rand(4, 2), count, criterion)


def test_a_count_in_range_reaches_information():
    """1 and N pass the checks: the stub has no information(), which is the next thing most_informative touches"""
    from gdrf_amd.models import SparseMultinomialGDRF as G
    for count in (1, 4):
        with pytest.raises(AttributeError, match="information"):
            G.most_informative(Stub, torch.rand(4, 2), count)


def test_information_with_a_custom_link_is_not_implemented():
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Linked(Stub):
        _link_function = staticmethod(lambda mu: torch.softmax(mu, -2))
    with pytest.raises(NotImplementedError, match="link_function"):
        G.information(Linked, torch.rand(4, 2), 8)
