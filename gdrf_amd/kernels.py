"""Stand-ins for the pyro.contrib.gp.kernels objects the reference builds in
gdrf/train_script.py:93-99,289-298 (``KERNEL_DICT[name](input_dim=, lengthscale=, variance=)``).

They only carry the hyper-parameters into the model; the covariance arithmetic is the HIP
kernels' (gdrf_amd/csrc/common.h::cov_from_r2; pyro semantics restated in SURVEY.md A.3).
"""
from __future__ import annotations

import torch


class Kernel:
    name = None
    kernel_id = None

    def __init__(self, input_dim: int, variance=None, lengthscale=None, active_dims=None):
        if active_dims is not None and list(active_dims) != list(range(input_dim)):
            raise NotImplementedError("active_dims other than all input dimensions")
        self.input_dim = int(input_dim)
        self.variance = torch.as_tensor(1.0 if variance is None else variance, dtype=torch.float64).detach().cpu().reshape(())
        self.lengthscale = self._lengthscale(lengthscale, self.input_dim)
        if not (self.variance > 0 and bool((self.lengthscale > 0).all())):
            raise ValueError("variance and lengthscale must be positive")

    @staticmethod
    def _lengthscale(lengthscale, input_dim: int) -> torch.Tensor:
        """One element (shape () or (1,)): the isotropic kernel, stored with shape ().  ``input_dim`` elements along one axis: one
        lengthscale per input dimension (ARD), stored with shape (input_dim,) - pyro's Isotropy._scale divides each input axis by its
        own entry.  Any other shape is an error."""
        t = torch.as_tensor(1.0 if lengthscale is None else lengthscale, dtype=torch.float64).detach().cpu()
        if t.dim() <= 1 and t.numel() == 1:
            return t.reshape(())
        if t.dim() == 1 and t.numel() == input_dim:
            return t.clone()
        raise ValueError(f"lengthscale must have 1 or input_dim = {input_dim} elements along one axis, got shape {tuple(t.shape)}")

    @property
    def ard(self) -> bool:
        """One lengthscale per input dimension."""
        return self.lengthscale.dim() == 1

    def to(self, device):
        return self

    def __repr__(self):
        ls = self.lengthscale.tolist() if self.ard else float(self.lengthscale)
        return f"{type(self).__name__}(input_dim={self.input_dim}, lengthscale={ls}, variance={float(self.variance)})"


class RBF(Kernel):
    name = "rbf"
    kernel_id = 0


class Matern52(Kernel):
    name = "matern52"
    kernel_id = 1


class Matern32(Kernel):
    name = "matern32"
    kernel_id = 2


class Exponential(Kernel):
    name = "exponential"
    kernel_id = 3


class RationalQuadratic(Kernel):
    """variance * (1 + r2 / (2 scale_mixture))^(-scale_mixture); scale_mixture is a third positive, learnable
    hyper-parameter (pyro.contrib.gp.kernels.RationalQuadratic(input_dim, variance, lengthscale, scale_mixture))."""
    name = "rationalquadratic"
    kernel_id = 4

    def __init__(self, input_dim: int, variance=None, lengthscale=None, scale_mixture=None, active_dims=None):
        super().__init__(input_dim, variance=variance, lengthscale=lengthscale, active_dims=active_dims)
        self.scale_mixture = torch.as_tensor(1.0 if scale_mixture is None else scale_mixture,
                                             dtype=torch.float64).detach().cpu().reshape(())
        if not self.scale_mixture > 0:
            raise ValueError("scale_mixture must be positive")


class Periodic(Kernel):
    """pyro.contrib.gp.kernels.Periodic: variance * exp(-2 sum_d sin^2(pi (x_d - z_d) / period_d) / lengthscale_d^2).  ``period`` is
    positive and learnable, one element or ``input_dim`` elements (one per input axis), in the scaled units the model sees (the unit
    cube of its ``world``).  Up to two input dimensions (the device evaluates it on two embedded coordinates per axis)."""
    name = "periodic"
    kernel_id = 5

    def __init__(self, input_dim: int, variance=None, lengthscale=None, period=None, active_dims=None):
        super().__init__(input_dim, variance=variance, lengthscale=lengthscale, active_dims=active_dims)
        t = torch.as_tensor(1.0 if period is None else period, dtype=torch.float64).detach().cpu()
        if t.dim() <= 1 and t.numel() == 1:
            t = t.reshape(())
        elif t.dim() == 1 and t.numel() == self.input_dim:
            t = t.clone()
        else:
            raise ValueError(f"period must have 1 or input_dim = {self.input_dim} elements along one axis, got shape {tuple(t.shape)}")
        if not bool((t > 0).all()):
            raise ValueError("period must be positive")
        self.period = t

    def __repr__(self):
        p = self.period.tolist() if self.period.dim() == 1 else float(self.period)
        return super().__repr__()[:-1] + f", period={p})"


KERNEL_DICT = {"rbf": RBF, "matern32": Matern32, "matern52": Matern52, "exponential": Exponential,
               "rationalquadratic": RationalQuadratic}
