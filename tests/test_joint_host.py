"""CPU tests of the joint-posterior surface (csrc/predict_cov.h): the library exports its entry points, and the argument errors are
raised before any device call (a model cannot be built without a HIP device, so its methods are called unbound on a stub)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stub:
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    K, _K, M, _link_function = 3, 3, 7, None


def test_library_exports_the_entry_points(hip_lib):
    from gdrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    for name, nargs in (("gdrf_predict_cov", 8), ("gdrf_sample_joint", 12), ("gdrf_sample_joint_retry", 6),
                        ("gdrf_joint_failed", 3)):
        assert hasattr(hip_lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"\bint %s\(gdrf_ctx\* ctx," % name, header)
    assert "GDRF_COV_FULL = 0, GDRF_COV_RESID = 1" in header


def test_the_methods_exist_on_the_model_and_on_a_snapshot():
    from gdrf_amd.engine import Engine
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        for name in ("posterior", "sample_fields", "sample_topic_maps"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Engine.predict_cov) and callable(Engine.sample_joint)
    assert Engine.last_joint_jitter is None


def test_check_joint_args_accepts_what_it_should():
    from gdrf_amd.engine import JOINT_MAX_ROWS, check_joint_args
    assert check_joint_args(1, 3, 7, 1) == 1
    assert check_joint_args(5, 3, 7, JOINT_MAX_ROWS) == 5
    assert check_joint_args(2.0, 3, 7, 4) == 2 and isinstance(check_joint_args(2.0, 3, 7, 4), int)
    assert check_joint_args(2, 3, 7, 4, xi=torch.zeros(2, 3, 7), zeta=torch.zeros(2, 3, 4)) == 2
    assert check_joint_args(2, 3, 7, 4, xi=torch.zeros(2, 3, 7)) == 2 and check_joint_args(2, 3, 7, 4, zeta=torch.zeros(2, 3, 4)) == 2


@pytest.mark.parametrize("num_samples", [0, -3, 2.5, True])
def test_num_samples_must_be_a_positive_integer(num_samples):
    from gdrf_amd.engine import Engine, check_joint_args
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="num_samples"):
        check_joint_args(num_samples, 3, 7, 4)
    with pytest.raises(ValueError, match="num_samples"):
        G.sample_fields(Stub, torch.rand(4, 2), num_samples)
    with pytest.raises(ValueError, match="num_samples"):
        G.sample_topic_maps(Stub, torch.rand(4, 2), num_samples)
    with pytest.raises(ValueError, match="num_samples"):
        Engine.sample_joint(Stub, torch.rand(4, 2), num_samples, seed=1)


@pytest.mark.parametrize("shape", [(2, 3, 4), (2, 4, 7), (3, 3, 7), (2, 21), (2 * 3 * 7,)])
def test_an_xi_of_another_shape_is_a_value_error(shape):
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="xi"):
        G.sample_fields(Stub, torch.rand(4, 2), 2, xi=torch.zeros(shape))          # (S, K, M) = (2, 3, 7)
    with pytest.raises(ValueError, match="xi"):
        Engine.sample_joint(Stub, torch.rand(4, 2), 2, xi=torch.zeros(shape))


@pytest.mark.parametrize("shape", [(2, 3, 7), (2, 4, 4), (3, 3, 4), (2, 12), (2 * 3 * 4,)])
def test_a_zeta_of_another_shape_is_a_value_error(shape):
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="zeta"):
        G.sample_fields(Stub, torch.rand(4, 2), 2, zeta=torch.zeros(shape))        # (S, K, n) = (2, 3, 4)
    with pytest.raises(ValueError, match="zeta"):
        Engine.sample_joint(Stub, torch.rand(4, 2), 2, xi=torch.zeros(2, 3, 7), zeta=torch.zeros(shape))


def test_the_row_cap_is_a_value_error_with_the_engine_untouched():
    """Stub has no engine, no device and no _prepare_inputs: reaching for any of them would be an AttributeError, not a ValueError"""
    from gdrf_amd.engine import JOINT_MAX_ROWS, Engine, check_joint_args
    from gdrf_amd.models import SparseMultinomialGDRF as G
    xs = torch.zeros(JOINT_MAX_ROWS + 1, 2)
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        check_joint_args(1, 3, 7, JOINT_MAX_ROWS + 1)
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        G.posterior(Stub, xs)
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        G.sample_fields(Stub, xs, 2)
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        G.sample_topic_maps(Stub, xs, 2)
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        Engine.predict_cov(Stub, xs, 0)
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        Engine.sample_joint(Stub, xs, 2, seed=1)
    with pytest.raises(ValueError, match="at least one row"):
        check_joint_args(1, 3, 7, 0)
    with pytest.raises(ValueError, match="which"):
        Engine.predict_cov(Stub, torch.zeros(4, 2), 2)


def test_forward_full_cov_points_to_posterior():
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(NotImplementedError, match=r"posterior\(Xnew\) returns"):
        G.forward(Stub, torch.rand(4, 2), full_cov=True)
