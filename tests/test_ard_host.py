"""ARD (one lengthscale per input dimension) on the host side: the kernel objects and train()'s argument check.  No GPU."""
import pytest
import torch

from gdrf_amd.kernels import KERNEL_DICT
from gdrf_amd.train import kernel_lengthscale_arg


@pytest.mark.parametrize("name", sorted(KERNEL_DICT))
@pytest.mark.parametrize("D", [2, 3, 4])
def test_kernel_accepts_one_lengthscale_per_dimension(name, D):
    ls = [0.12, 0.35, 0.2, 0.5][:D]
    for arg in (torch.tensor(ls, dtype=torch.float64), ls, tuple(ls)):
        k = KERNEL_DICT[name](input_dim=D, lengthscale=arg, variance=torch.tensor(2.0))
        assert k.ard
        assert k.lengthscale.shape == (D,) and k.lengthscale.dtype == torch.float64
        assert torch.equal(k.lengthscale, torch.tensor(ls, dtype=torch.float64))
        assert str(ls[1]) in repr(k)


@pytest.mark.parametrize("name", sorted(KERNEL_DICT))
@pytest.mark.parametrize("D", [1, 2, 3])
def test_one_element_keeps_the_scalar_form(name, D):
    for arg in (0.3, torch.tensor(0.3, dtype=torch.float64), torch.tensor([0.3], dtype=torch.float64), [0.3]):
        k = KERNEL_DICT[name](input_dim=D, lengthscale=arg)
        assert not k.ard
        assert k.lengthscale.shape == () and float(k.lengthscale) == 0.3
        assert repr(k) == f"{type(k).__name__}(input_dim={D}, lengthscale=0.3, variance=1.0)"


@pytest.mark.parametrize("name", sorted(KERNEL_DICT))
def test_bad_lengthscales_raise(name):
    cls = KERNEL_DICT[name]
    for bad in ([0.1, 0.2, 0.3], [0.1, 0.2, 0.3, 0.4, 0.5], torch.ones(2, 2), torch.ones(1, 2), torch.ones(2, 1), torch.ones(1, 1)):
        with pytest.raises(ValueError):
            cls(input_dim=2, lengthscale=bad)
    for bad in ([0.1, 0.0], [0.1, -0.2], 0.0, -1.0, [float("nan"), 0.1]):
        with pytest.raises(ValueError):
            cls(input_dim=2, lengthscale=bad)


def test_train_accepts_a_lengthscale_per_dimension():
    assert kernel_lengthscale_arg(0.1, 2).shape == ()
    assert kernel_lengthscale_arg([0.1], 2).shape == (1,)
    assert torch.equal(kernel_lengthscale_arg([0.05, 0.2], 2), torch.tensor([0.05, 0.2], dtype=torch.float64))
    assert kernel_lengthscale_arg((0.1, 0.2, 0.3), 3).shape == (3,)
    for bad, D in (([0.1, 0.2, 0.3], 2), ([0.1, 0.2], 3), ([[0.1, 0.2]], 2)):
        with pytest.raises(ValueError):
            kernel_lengthscale_arg(bad, D)
