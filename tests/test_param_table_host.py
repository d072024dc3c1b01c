"""The one description of a context's learnt parameters, without a GPU: gdrf_amd.engine.param_table on hand-made layout numbers, and the
factors() / params every kernel class reports (what the model's initialisation and the checkpoints walk)."""
import math

import pytest
import torch

from gdrf_amd.engine import Engine, param_table
from gdrf_amd.kernels import RBF, Exponential, Matern32, Matern52, Periodic, Product, RationalQuadratic, embedded_coordinates

K, M, V = 3, 4, 5
BASE = ["log_noise", "u_loc", "phi_unc", "u_scale_tril_unc"]
NESTED = [dict(name="kern0.kern0", kind="rbf", active_dims=[0], lengthscales=1, periods=0),
          dict(name="kern0.kern1", kind="periodic", active_dims=[1], lengthscales=1, periods=1),
          dict(name="kern1", kind="rbf", active_dims=[2], lengthscales=1)]
LONE = [dict(name="", kind="periodic", active_dims=[0, 1], lengthscales=2, periods=1)]      # four embedded coordinates, the most a context holds
MEANS = {"_mean_function.a": (), "_mean_function.w": (3, 2)}

# name: (D, param_table's keyword arguments, the expected names in order, the expected shapes of the kernel's own entries)
CONFIGS = {
    "isotropic": (2, dict(kernel="matern52"), ["log_lengthscale", "log_variance"] + BASE, {"log_lengthscale": ()}),
    "rationalquadratic": (2, dict(kernel="rationalquadratic"), ["log_lengthscale", "log_variance"] + BASE + ["log_scale_mixture"],
                          {"log_scale_mixture": ()}),
    "ard_d3": (3, dict(ard=True), ["log_lengthscale", "log_variance"] + BASE, {"log_lengthscale": (3,)}),
    "periodic_1": (2, dict(kernel="periodic", period_count=1), ["log_lengthscale", "log_variance"] + BASE + ["log_period"], {"log_period": ()}),
    "periodic_d": (2, dict(kernel="periodic", period_count=2, ard=True), ["log_lengthscale", "log_variance"] + BASE + ["log_period"],
                   {"log_period": (2,), "log_lengthscale": (2,)}),
    "nested_product": (3, dict(kernel="product", product=NESTED),
                       ["kern0.kern0.log_variance", "kern0.kern0.log_lengthscale", "kern0.kern1.log_variance", "kern0.kern1.log_lengthscale",
                        "kern0.kern1.log_period", "kern1.log_variance", "kern1.log_lengthscale"] + BASE,
                       {"kern0.kern1.log_period": ()}),
    "lone_factor": (3, dict(kernel="product", product=LONE), ["log_variance", "log_lengthscale", "log_period"] + BASE,
                    {"log_lengthscale": (2,), "log_period": ()}),
    "learn_inducing": (2, dict(learn_inducing=True), ["log_lengthscale", "log_variance"] + BASE + ["inducing_unc"], {"inducing_unc": (M, 2)}),
    "mean_params": (2, dict(mean_shapes=MEANS), ["log_lengthscale", "log_variance"] + BASE + list(MEANS),
                    {"_mean_function.a": (), "_mean_function.w": (3, 2)}),
}


def hand_made_raw(D, kw):
    """Layout numbers as a library could report them: the four scalar slots, the three blocks of every context, then one segment each for
    the inducing inputs, the ARD lengthscales / a product's three segments, the periods and the mean parameters."""
    o = 4
    lay = [0, 1, 2]
    for n in (K * M, K * V, K * M * M):
        lay.append(o)
        o += n
    raw = dict(inducing=(o, M * D))
    o += M * D
    prod = kw.get("product")
    if prod:
        nl, npr = sum(f["lengthscales"] for f in prod), sum(f.get("periods", 0) for f in prod)
        raw["product"] = (o, len(prod), o + len(prod), nl, o + len(prod) + nl, npr)
        o += len(prod) + nl + npr
    else:
        raw["ard"] = (o, D if kw.get("ard") else 0)
        o += raw["ard"][1]
        raw["periodic"] = (o, kw.get("period_count", 0))
        o += raw["periodic"][1]
    raw["mean"] = (o, sum(math.prod(s) for s in kw.get("mean_shapes", {}).values()))
    raw["param"] = tuple(lay) + (o + raw["mean"][1],)
    return raw


@pytest.mark.parametrize("name", list(CONFIGS))
def test_names_order_shapes_and_disjoint_segments(name):
    D, kw, names, shapes = CONFIGS[name]
    raw = hand_made_raw(D, kw)
    table = param_table(K, M, V, D, raw=raw, **kw)
    assert list(table) == names
    want = {n: () for n in names}              # every entry is a scalar but the three blocks and what the configuration says
    want.update(u_loc=(K, M), phi_unc=(K, V), u_scale_tril_unc=(K, M, M), **shapes)
    assert {n: shape for n, (_, shape) in table.items()} == want
    total = raw["param"][6]
    taken = sorted((o, o + math.prod(shape)) for o, shape in table.values())
    assert taken[0][0] >= 0 and taken[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:])), taken
    assert table["u_loc"][0] == 4 and table["log_noise"][0] == 2


def test_engine_reads_the_table():
    """view(), param_names, named_views() and segments() of an engine are lookups in its table (a host stand-in: CPU buffers)."""
    D, kw, names, _ = CONFIGS["nested_product"]
    raw = hand_made_raw(D, kw)
    eng = Engine.__new__(Engine)
    eng.product, eng.table = kw["product"], param_table(K, M, V, D, raw=raw, **kw)
    eng.params = torch.arange(raw["param"][6], dtype=torch.float64)
    assert list(eng.param_names) == names == list(eng.named_views())
    for n, (o, shape) in eng.table.items():
        v = eng.view(n)
        assert tuple(v.shape) == shape and v.data_ptr() == eng.params.data_ptr() + 8 * o
        assert torch.equal(v.flatten(), eng.params[o:o + math.prod(shape)])
    assert eng.segments() == {n: (o, math.prod(shape)) for n, (o, shape) in eng.table.items()}
    with pytest.raises(KeyError, match="a product context's kernel parameters are .*kern0.kern0.log_variance.*kern1.log_lengthscale"):
        eng.view("log_lengthscale")
    with pytest.raises(KeyError):
        eng.view("inducing_unc")                 # not learnt here


def test_factors_and_params_of_every_kernel_class():
    for cls in (RBF, Matern52, Matern32, Exponential):
        k = cls(2)
        assert k.factors() == [("", k)] and k.params == ("variance", "lengthscale") and embedded_coordinates(k) == 2
    rq = RationalQuadratic(2, scale_mixture=1.3)
    assert rq.factors() == [("", rq)] and rq.params == ("variance", "lengthscale", "scale_mixture")
    per = Periodic(2, period=[0.3, 0.4])
    assert per.factors() == [("", per)] and per.params == ("variance", "lengthscale", "period") and embedded_coordinates(per) == 4
    for k in (rq, per):
        assert all(bool((getattr(k, n) > 0).all()) for n in k.params)
    a, b, c = RBF(1, active_dims=[0]), Periodic(1, active_dims=[1]), RBF(1, active_dims=[1])
    prod = Product(Product(a, b), c)
    assert prod.factors() == [("kern0.kern0", a), ("kern0.kern1", b), ("kern1", c)] and prod.params == ()
    assert embedded_coordinates(prod) == 1 + 2 + 1
