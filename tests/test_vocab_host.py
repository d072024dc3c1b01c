"""CPU tests of the rows_form argument (the vocabulary-streamed row form, csrc/rows_vstream.h): the library exports its entry points
and the model surface rejects an unknown form before it touches the GPU."""
import inspect

import pytest
import torch


def test_library_exports_the_rows_form_entry_points(hip_lib):
    from gdrf_amd import _lib
    for name in ("gdrf_set_rows_form", "gdrf_get_rows_form"):
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name), name


def test_rows_form_is_a_keyword_of_engine_model_and_train():
    from gdrf_amd.engine import Engine
    from gdrf_amd.models import SparseMultinomialGDRF
    from gdrf_amd.train import train
    for fn in (Engine.__init__, SparseMultinomialGDRF.__init__, train):
        p = inspect.signature(fn).parameters["rows_form"]
        assert p.default == "auto", fn


@pytest.mark.parametrize("form", ["bogus", "lds", "", None, 1])
def test_model_rejects_an_unknown_rows_form_before_touching_the_gpu(form):
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    xs, ws = torch.rand(10, 2), torch.randint(0, 3, (10, 5))
    with pytest.raises(ValueError, match="rows_form"):
        SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2,
                              kernel=RBF(input_dim=2, lengthscale=torch.tensor(0.2), variance=torch.tensor(1.0)),
                              num_observation_categories=5, num_topic_categories=2, dirichlet_param=0.01, n_points=[2, 2],
                              device="cpu", rows_form=form)
