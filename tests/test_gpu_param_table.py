"""GPU: an engine's parameter table against the library's own layout calls, for the configurations of tests/test_param_table_host.py, and
checkpoints written before every snapshot carried a kernel_spec."""
import copy
import ctypes as C
import math

import pytest
import torch

from gdrf_amd.data import synth_circles
from tests.test_param_table_host import CONFIGS

pytestmark = pytest.mark.gpu

K, M, V = 3, 12, 7


def _layout(eng, name, size):
    out = (C.c_int64 * size)()
    assert getattr(eng.lib, name)(eng.ctx, out) == 0
    return tuple(out)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_table_against_the_library(name):
    from gdrf_amd.engine import Engine
    D, kw, names, _ = CONFIGS[name]
    kw = dict(kw)
    mean_shapes = kw.pop("mean_shapes", None)
    eng = Engine(144, M, K, V, D, dtype=torch.float64, process_group=None, mean_params=mean_shapes, **kw)
    t = eng.table
    assert list(t) == names == list(eng.param_names)
    start = lambda n: t[n][0]
    count = lambda ns: sum(math.prod(t[n][1]) for n in ns)
    lay = _layout(eng, "gdrf_param_layout", 7)
    assert (start("log_noise"), start("u_loc"), start("phi_unc"), start("u_scale_tril_unc")) == lay[2:6] and eng.layout["total"] == lay[6]
    if eng.product is None:
        al = _layout(eng, "gdrf_ard_layout", 2)
        assert start("log_variance") == lay[1] and start("log_lengthscale") == (al[0] if eng.ard else lay[0])
        assert al[1] == (D if eng.ard else 0)
    else:
        pl = _layout(eng, "gdrf_product_layout", 6)
        for leaf, (o, n) in (("log_variance", pl[0:2]), ("log_lengthscale", pl[2:4]), ("log_period", pl[4:6])):
            seg = [x for x in names if x.rpartition(".")[2] == leaf]
            assert count(seg) == n and (not seg or start(seg[0]) == o)
            for a, b in zip(seg, seg[1:]):                       # the factors' entries follow each other in factor order
                assert start(b) == start(a) + math.prod(t[a][1])
    if eng.period_count:
        assert (start("log_period"), count(["log_period"])) == _layout(eng, "gdrf_periodic_layout", 2)
    if eng.learn_inducing:
        assert (start("inducing_unc"), count(["inducing_unc"])) == _layout(eng, "gdrf_inducing_layout", 2)
    if mean_shapes:
        ml = _layout(eng, "gdrf_mean_param_layout", 2)
        assert (start(next(iter(mean_shapes))), count(mean_shapes)) == ml and eng.layout["mean"] == ml[0]
        o = ml[0]
        for n, shape in mean_shapes.items():
            assert t[n] == (o, tuple(shape))
            o += math.prod(shape)
    taken = sorted((o, o + math.prod(shape)) for o, shape in t.values())
    assert taken[0][0] >= 0 and taken[-1][1] <= lay[6] and all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))
    for n, (o, shape) in t.items():
        v = eng.view(n)
        assert tuple(v.shape) == shape and v.data_ptr() == eng.params.data_ptr() + o * eng.params.element_size(), n
        assert eng.layout[n] == o
    assert eng.segments() == {n: (o, math.prod(shape)) for n, (o, shape) in t.items()}


def _model(kernel):
    from gdrf_amd.models import SparseMultinomialGDRF
    xs, ws, _ = synth_circles(16, 9, V, K, seed=1)
    model = SparseMultinomialGDRF(xs=torch.from_numpy(xs).double().cuda(), ws=torch.from_numpy(ws).int().cuda(), world=[(0.0, 1.0)] * 2,
                                  kernel=kernel, num_observation_categories=V, num_topic_categories=K, dirichlet_param=0.01, n_points=[4, 3],
                                  jitter=1e-6, device="cuda:0", dtype=torch.float64, seed=3)
    g = torch.Generator().manual_seed(7)                         # values no initialisation would give
    model._engine.params.add_(0.1 * torch.randn(model._engine.params.shape, generator=g, dtype=torch.float64).cuda())
    return model


@pytest.mark.parametrize("kind", ["ard_rbf", "per_axis_periodic"])
@pytest.mark.parametrize("legacy", ["absent", "none"])
def test_checkpoint_without_a_kernel_spec_restores_to_the_bit(kind, legacy):
    from gdrf_amd.kernels import RBF, Periodic
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot
    kernel = RBF(2, lengthscale=[0.15, 0.3], variance=25.0) if kind == "ard_rbf" else Periodic(2, lengthscale=[0.6, 0.9], period=[0.4, 0.7])
    model = _model(kernel)
    snap = copy.deepcopy(model)
    assert snap.meta["kernel_spec"]["kind"] == kernel.name
    meta = dict(snap.meta)
    if legacy == "absent":
        del meta["kernel_spec"]
    else:
        meta["kernel_spec"] = None
    re = ModelSnapshot(snap.state_dict(), meta).restore()
    assert type(re._kernel) is type(kernel) and re._engine.ard and re._engine.period_count == model._engine.period_count
    sd, want = re.state_dict(), model.state_dict()
    assert list(sd) == list(want)
    for k in want:
        assert sd[k].shape == want[k].shape and torch.equal(sd[k], want[k]), k
