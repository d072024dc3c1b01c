"""CPU tests of the batch-choice surface (csrc/select_batch.h): the library exports its entry point, the methods exist, and the argument
errors are raised before any device call (a model cannot be built without a HIP device, so its methods are called unbound on a stub)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stub:
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs, noise) is an AttributeError"""
    K, _K, M, _link_function = 3, 3, 7, None


def test_library_exports_the_entry_point(hip_lib):
    from gdrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert hasattr(hip_lib, "gdrf_select_batch")
    assert len(_lib.SIGNATURES["gdrf_select_batch"][1]) == 13
    decl = re.search(r"\bint gdrf_select_batch\(gdrf_ctx\* ctx,([^;]*)\);", header)
    assert decl and decl.group(1).count(",") + 2 == 13           # the header's argument count
    assert "#define GDRF_SELECT_MAX_PICKS 256" in header


def test_the_methods_exist_on_the_model_the_snapshot_and_the_engine():
    from gdrf_amd.engine import SELECT_MAX_PICKS, Engine, check_select_args
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot, Engine):
        assert callable(getattr(cls, "select_batch")), cls
    assert SELECT_MAX_PICKS == 256 and callable(check_select_args)
    assert "select_batch" in SparseMultinomialGDRF.most_informative.__doc__


def test_check_select_args_accepts_what_it_should():
    from gdrf_amd.engine import SELECT_MAX_PICKS, check_select_args
    assert check_select_args(1, 0.5, 1) == (1, 0.5, 0)
    assert check_select_args(4, 1e-3, 4) == (4, 1e-3, 0)
    c, s2, G = check_select_args(3.0, 2, 10)
    assert (c, s2, G) == (3, 2.0, 0) and isinstance(c, int) and isinstance(s2, float)
    assert check_select_args(3, None, 10) == (3, None, 0)                            # the model fills in its own noise
    assert check_select_args(3, 0.5, 10, given=torch.zeros(5, 2), dims=2) == (3, 0.5, 5)
    assert check_select_args(3, 0.5, 10, given=torch.zeros(0, 2), dims=2) == (3, 0.5, 0)
    assert check_select_args(SELECT_MAX_PICKS, 0.5, 300) == (SELECT_MAX_PICKS, 0.5, 0)
    assert check_select_args(SELECT_MAX_PICKS - 5, 0.5, 300, given=torch.zeros(5, 2), dims=2)[2] == 5


def raises_everywhere(match, xs, count, noise=0.5, given=None):
    from gdrf_amd.engine import Engine, check_select_args
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match=match):
        check_select_args(count, noise, int(xs.shape[0]), given, int(xs.shape[1]))
    with pytest.raises(ValueError, match=match):
        G.select_batch(Stub, xs, count, noise=noise, given=given)
    with pytest.raises(ValueError, match=match):
        Engine.select_batch(Stub, xs, count, noise, given=given)


@pytest.mark.parametrize("count", [0, -2, 2.5, True, 5])
def test_count_must_be_an_integer_between_one_and_the_rows(count):
    raises_everywhere("count", torch.rand(4, 2), count)


def test_the_given_rows_and_the_picks_share_the_cap():
    from gdrf_amd.engine import SELECT_MAX_PICKS
    xs = torch.rand(SELECT_MAX_PICKS + 44, 2)
    raises_everywhere("SELECT_MAX_PICKS", xs, SELECT_MAX_PICKS + 1)
    raises_everywhere("SELECT_MAX_PICKS", xs, SELECT_MAX_PICKS - 4, given=torch.rand(5, 2))


@pytest.mark.parametrize("noise", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_noise_must_be_positive_and_finite(noise):
    raises_everywhere("noise", torch.rand(4, 2), 2, noise=noise)


@pytest.mark.parametrize("shape", [(3, 1), (3, 3), (6,), (1, 3, 2)])
def test_a_given_with_other_columns_is_a_value_error(shape):
    raises_everywhere("given", torch.rand(4, 2), 2, given=torch.zeros(shape))


def test_the_engine_needs_a_noise():
    from gdrf_amd.engine import Engine
    with pytest.raises(ValueError, match="noise"):
        Engine.select_batch(Stub, torch.rand(4, 2), 2, None)
