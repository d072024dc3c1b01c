"""Products of RBF and Periodic kernels and active_dims on the host side: construction, validation, the embedded-coordinate table, the
model's limits and the parameter names.  No GPU."""
import pytest
import torch

from gdrf_amd.kernels import KERNEL_DICT, RBF, Matern32, Matern52, Exponential, Periodic, Product, RationalQuadratic, Sum, \
    embedded_coordinates
from gdrf_amd.models.sparse_gdrf import _PARAM_KEYS, kernel_from_spec, kernel_spec, product_table, state_key
from gdrf_amd.optim import param_store_name


def test_active_dims_follow_pyro():
    assert RBF(2).active_dims == [0, 1] and not RBF(2).explicit_active_dims
    k = RBF(2, active_dims=[0, 2], lengthscale=[0.3, 0.4])
    assert k.active_dims == [0, 2] and k.explicit_active_dims and k.lengthscale.shape == (2,)
    assert Periodic(1, active_dims=[2], period=0.5).active_dims == [2]
    with pytest.raises(ValueError):
        RBF(2, active_dims=[0])                      # input_dim == len(active_dims)
    with pytest.raises(ValueError):
        Periodic(1, active_dims=[0, 1])
    with pytest.raises(ValueError):
        RBF(2, active_dims=[1, 1])
    with pytest.raises(ValueError):
        RBF(1, active_dims=[1], lengthscale=[0.3, 0.4])    # one value per active dim


@pytest.mark.parametrize("cls", [Matern32, Matern52, Exponential, RationalQuadratic])
def test_other_kinds_refuse_a_proper_subset(cls):
    with pytest.raises(NotImplementedError):
        cls(1, active_dims=[1])
    assert cls(2, active_dims=[0, 1]).active_dims == [0, 1]


def test_product_union_and_nesting():
    p = Product(RBF(2, active_dims=[0, 1]), Periodic(1, active_dims=[2]))
    assert p.active_dims == [0, 1, 2] and p.input_dim == 3 and p.name == "product"
    q = Product(Product(RBF(1, active_dims=[3]), RBF(1, active_dims=[0])), Periodic(1, active_dims=[0]))
    assert q.active_dims == [0, 3] and q.input_dim == 2
    assert [path for path, _ in q.factors()] == ["kern0.kern0", "kern0.kern1", "kern1"]
    assert q.kern0.kern1.active_dims == [0]
    assert "product" not in KERNEL_DICT and Product not in KERNEL_DICT.values() and len(KERNEL_DICT) == 5


def test_unsupported_factors():
    with pytest.raises(NotImplementedError, match="constant"):
        Product(RBF(1), 2.0)
    with pytest.raises(NotImplementedError, match="constant"):
        Product(RBF(1), torch.tensor(2.0))
    with pytest.raises(NotImplementedError, match="RBF, Periodic or Product"):
        Product(RBF(1), Matern32(1))
    with pytest.raises(NotImplementedError, match="Sum"):
        Sum(RBF(1), RBF(1))
    with pytest.raises(NotImplementedError):
        Product(RBF(1), object())


def _table(kernel, D):
    return [(f["name"], f["kind"], f["active_dims"], f["lengthscales"], f["periods"]) for f in product_table(kernel, D)]


def test_factor_tables_and_coordinates():
    lp = Product(RBF(1, lengthscale=2.0), Periodic(1, period=0.3))
    assert _table(lp, 1) == [("kern0", "rbf", [0], 1, 0), ("kern1", "periodic", [0], 1, 1)] and embedded_coordinates(lp) == 3
    st = Product(RBF(2, active_dims=[0, 1], lengthscale=[0.3, 0.5]), Periodic(1, active_dims=[2], period=0.25))
    assert _table(st, 3) == [("kern0", "rbf", [0, 1], 2, 0), ("kern1", "periodic", [2], 1, 1)] and embedded_coordinates(st) == 4
    pp = Product(Periodic(1, active_dims=[0]), Periodic(1, active_dims=[1], lengthscale=0.7))
    assert embedded_coordinates(pp) == 4
    # a lone RBF or Periodic on a proper subset runs as a one-factor product named like the lone kernel
    assert _table(Periodic(1, active_dims=[1], period=0.5), 2) == [("", "periodic", [1], 1, 1)]
    assert _table(RBF(2, active_dims=[2, 0]), 3) == [("", "rbf", [2, 0], 1, 0)]
    # all axes: the kernel's own kind
    assert product_table(RBF(2), 2) is None and product_table(RBF(2, active_dims=[0, 1]), 2) is None
    assert product_table(Periodic(2), 2) is None


def _model(kernel, D):
    from gdrf_amd.models import SparseMultinomialGDRF
    xs = torch.rand(10, D)
    ws = torch.randint(0, 3, (10, 5), dtype=torch.int32)
    return SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * D, kernel=kernel, num_observation_categories=5,
                                 num_topic_categories=2, dirichlet_param=0.01, n_points=[2] * D, device="cpu")


@pytest.mark.parametrize("kernel,D", [
    (Periodic(3, active_dims=[0, 1, 2]), 4),
    (Product(RBF(3, active_dims=[0, 1, 2]), Periodic(1, active_dims=[3])), 4),
    (Product(Periodic(1, active_dims=[0]), Product(Periodic(1, active_dims=[1]), RBF(1, active_dims=[0]))), 2),
])
def test_more_than_four_coordinates_are_refused_before_the_gpu(kernel, D):
    with pytest.raises(ValueError, match="at most 4"):
        _model(kernel, D)


def test_active_dims_outside_the_world_are_refused():
    with pytest.raises(ValueError, match="not axes"):
        _model(Product(RBF(1, active_dims=[0]), Periodic(1, active_dims=[2])), 2)


def test_whole_periodic_keeps_its_limit():
    with pytest.raises(ValueError, match="at most 2 input dimensions"):
        _model(Periodic(3), 3)


def test_state_dict_and_param_store_names():
    assert state_key("kern0.log_variance") == "_kernel.kern0.variance_unconstrained"
    assert state_key("kern0.log_lengthscale") == "_kernel.kern0.lengthscale_unconstrained"
    assert state_key("kern1.log_period") == "_kernel.kern1.period_unconstrained"
    assert state_key("kern0.kern1.log_period") == "_kernel.kern0.kern1.period_unconstrained"
    assert state_key("log_period") == _PARAM_KEYS["log_period"] == "_kernel.period_unconstrained"
    assert state_key("u_loc") == "u_loc_unconstrained" and state_key("_mean_function.w") == "_mean_function.w"
    assert param_store_name("kern0.kern1.log_lengthscale") == "_kernel.kern0.kern1.lengthscale"
    assert param_store_name("kern1.log_variance") == "_kernel.kern1.variance"


def test_kernel_spec_round_trip_is_plain_values():
    k = Product(Product(RBF(2, active_dims=[0, 1], lengthscale=[0.3, 0.4]), RBF(1, active_dims=[2])),
                Periodic(1, active_dims=[2], period=0.2))
    spec = kernel_spec(k)

    def plain(v):
        return v is None or isinstance(v, (int, str)) or (isinstance(v, list) and all(plain(x) for x in v)) or \
            (isinstance(v, dict) and all(isinstance(a, str) and plain(b) for a, b in v.items()))
    assert plain(spec)
    back = kernel_from_spec(spec)
    assert _table(back, 3) == _table(k, 3)
    assert back.kern0.kern0.lengthscale.shape == (2,) and back.kern1.period.shape == ()
