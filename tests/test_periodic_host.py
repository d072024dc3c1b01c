"""The Periodic kernel on the host side: construction, validation, the model's dimension limit and KERNEL_DICT.  No GPU."""
import pytest
import torch

from gdrf_amd.kernels import KERNEL_DICT, Periodic


@pytest.mark.parametrize("D", [1, 2])
def test_scalar_and_per_axis_period_and_lengthscale(D):
    k = Periodic(D, variance=2.0, lengthscale=0.5, period=0.25)
    assert k.name == "periodic" and k.kernel_id == 5
    assert k.period.shape == () and float(k.period) == 0.25 and k.period.dtype == torch.float64
    assert k.lengthscale.shape == () and not k.ard
    per = [0.25, 0.5][:D]
    ls = [0.7, 1.1][:D]
    k = Periodic(D, lengthscale=ls, period=torch.tensor(per))
    shape = (D,) if D > 1 else ()                      # one element is the shared form, as for the lengthscale
    assert k.period.shape == shape and torch.equal(k.period.reshape(-1), torch.tensor(per, dtype=torch.float64))
    assert k.lengthscale.shape == shape and k.ard == (D > 1)
    for one in (0.3, [0.3], torch.tensor([0.3])):
        assert Periodic(D, period=one).period.shape == ()
    assert float(Periodic(D).period) == 1.0           # pyro's default: torch.tensor(1.0)


def test_repr_shows_the_period():
    assert repr(Periodic(1, lengthscale=0.5, period=0.25)) == "Periodic(input_dim=1, lengthscale=0.5, variance=1.0, period=0.25)"
    assert repr(Periodic(2, period=[0.25, 0.5])) == "Periodic(input_dim=2, lengthscale=1.0, variance=1.0, period=[0.25, 0.5])"


@pytest.mark.parametrize("bad", [0.0, -1.0, [0.2, -0.1], [0.2, 0.3, 0.4], [[0.2, 0.3]], torch.zeros(2)])
def test_bad_period_raises(bad):
    with pytest.raises(ValueError):
        Periodic(2, period=bad)


def test_three_dimensions_are_refused_before_the_gpu():
    from gdrf_amd.models import SparseMultinomialGDRF
    xs = torch.rand(10, 3)
    ws = torch.randint(0, 3, (10, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 2 input dimensions"):
        SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 3, kernel=Periodic(3, period=0.5), num_observation_categories=5,
                              num_topic_categories=2, dirichlet_param=0.01, n_points=[2, 2, 2], device="cpu")


def test_state_dict_key_and_kernel_dict_unchanged():
    from gdrf_amd.models.sparse_gdrf import _PARAM_KEYS
    assert _PARAM_KEYS["log_period"] == "_kernel.period_unconstrained"
    assert sorted(KERNEL_DICT) == ["exponential", "matern32", "matern52", "rationalquadratic", "rbf"]
    assert Periodic not in KERNEL_DICT.values()
