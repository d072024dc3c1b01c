"""Stand-ins for the pyro.contrib.gp.kernels objects the reference builds in
gdrf/train_script.py:93-99,289-298 (``KERNEL_DICT[name](input_dim=, lengthscale=, variance=)``).

They only carry the hyper-parameters into the model; the covariance arithmetic is the HIP
kernels' (gdrf_amd/csrc/common.h::cov_from_r2; pyro semantics restated in SURVEY.md A.3).
"""
from __future__ import annotations

import numbers

import torch


def _active_dims(input_dim: int, active_dims):
    """pyro 1.8 Kernel.__init__: None means the first ``input_dim`` axes; otherwise ``input_dim == len(active_dims)``."""
    if active_dims is None:
        return list(range(int(input_dim))), False
    dims = [int(d) for d in active_dims]
    if len(dims) != int(input_dim):
        raise ValueError("Input size and the length of active dimensionals should be equal.")
    if any(d < 0 for d in dims) or len(set(dims)) != len(dims):
        raise ValueError(f"active_dims must be distinct non-negative axes, got {dims}")
    return dims, True


class Kernel:
    name = None
    kernel_id = None
    subset_dims = False          # True for the kinds that may read a proper subset of the input axes (RBF, Periodic)
    params = ("variance", "lengthscale")      # a leaf's positive learnable parameters, in the order the engine names them ("log_" + name)
    coords_per_axis = 1                       # embedded coordinates the device evaluates each of its axes on

    def __init__(self, input_dim: int, variance=None, lengthscale=None, active_dims=None):
        self.active_dims, self.explicit_active_dims = _active_dims(input_dim, active_dims)
        if self.active_dims != list(range(int(input_dim))) and not self.subset_dims:
            raise NotImplementedError(f"{type(self).__name__} with active_dims other than all input dimensions: only RBF and Periodic "
                                      "take a subset of the axes")
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

    def factors(self, prefix: str = ""):
        """The leaf factors as [(path, kernel)]: a leaf is its own single factor, with the empty path."""
        return [("", self)]

    def __repr__(self):
        ls = self.lengthscale.tolist() if self.ard else float(self.lengthscale)
        return f"{type(self).__name__}(input_dim={self.input_dim}, lengthscale={ls}, variance={float(self.variance)})"


class RBF(Kernel):
    name = "rbf"
    kernel_id = 0
    subset_dims = True


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
    params = Kernel.params + ("scale_mixture",)

    def __init__(self, input_dim: int, variance=None, lengthscale=None, scale_mixture=None, active_dims=None):
        super().__init__(input_dim, variance=variance, lengthscale=lengthscale, active_dims=active_dims)
        self.scale_mixture = torch.as_tensor(1.0 if scale_mixture is None else scale_mixture,
                                             dtype=torch.float64).detach().cpu().reshape(())
        if not self.scale_mixture > 0:
            raise ValueError("scale_mixture must be positive")


class Periodic(Kernel):
    """pyro.contrib.gp.kernels.Periodic: variance * exp(-2 sum_d sin^2(pi (x_d - z_d) / period_d) / lengthscale_d^2).  ``period`` is
    positive and learnable, one element or ``input_dim`` elements (one per input axis), in the scaled units the model sees (the unit
    cube of its ``world``).  The device evaluates it on two embedded coordinates per axis, at most 4: a kernel over all the world's
    axes takes up to two; with ``active_dims`` or in a Product it shares the 4 with the other factors."""
    name = "periodic"
    kernel_id = 5
    subset_dims = True
    params = Kernel.params + ("period",)
    coords_per_axis = 2

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


class Product(Kernel):
    """pyro.contrib.gp.kernels.Product(kern0, kern1): kern0(X, Z) * kern1(X, Z), each factor reading its own ``active_dims`` of the
    inputs.  As in pyro 1.8's Combination, ``active_dims`` is the sorted union of the factors' and ``input_dim`` its length.  The factors
    are RBF, Periodic or Product kernels and keep their own learnable parameters (the product's variance is the product of theirs).  The
    device evaluates it on the factors' embedded coordinates (one per RBF axis, two per Periodic axis, at most 4 in all)."""
    name = "product"
    kernel_id = 6
    params = ()                  # its leaves hold them all

    def __init__(self, kern0, kern1):
        for k in (kern0, kern1):
            if isinstance(k, numbers.Number) or (isinstance(k, torch.Tensor) and k.dim() == 0):
                raise NotImplementedError("Product with a constant factor is not supported: scale a factor's variance instead")
            if not isinstance(k, (RBF, Periodic, Product)):
                raise NotImplementedError(f"Product factors must be RBF, Periodic or Product kernels, got {type(k).__name__}")
        self.kern0, self.kern1 = kern0, kern1
        self.active_dims = sorted(set(kern0.active_dims) | set(kern1.active_dims))
        self.input_dim = len(self.active_dims)
        self.explicit_active_dims = True

    @property
    def ard(self) -> bool:
        return False

    def factors(self, prefix: str = ""):
        """The leaf factors in pyro's module order: [(path, kernel)], path like "kern0.kern1"."""
        out = []
        for attr in ("kern0", "kern1"):
            k, path = getattr(self, attr), prefix + attr
            out += k.factors(path + ".") if isinstance(k, Product) else [(path, k)]
        return out

    def __repr__(self):
        return f"Product({self.kern0!r}, {self.kern1!r})"


class Sum(Kernel):
    """pyro.contrib.gp.kernels.Sum: not supported (a sum of kernels is no product of embedded RBF factors)."""
    name = "sum"

    def __init__(self, kern0, kern1):
        raise NotImplementedError("Sum of kernels is not supported; Product of RBF and Periodic factors is")


def embedded_coordinates(kernel) -> int:
    """The embedded coordinates the device evaluates ``kernel`` on: one per RBF axis, two per Periodic axis."""
    return sum(k.coords_per_axis * k.input_dim for _, k in kernel.factors())


KERNEL_DICT = {"rbf": RBF, "matern32": Matern32, "matern52": Matern52, "exponential": Exponential,
               "rationalquadratic": RationalQuadratic}
