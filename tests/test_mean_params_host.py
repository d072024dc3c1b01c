"""Trainable mean_function parameters on the host side: which callables count as learnable, the ``_mean_function.*`` names of the
state_dict and the optimizer state, strict and non-strict loading, and the device check.  No GPU: the engine below is a host-only
stand-in with the real Engine's naming and view methods over CPU buffers."""
import pytest
import torch

from gdrf_amd.engine import Engine, param_table
from gdrf_amd.models.sparse_gdrf import MEAN_PREFIX, SparseMultinomialGDRF, learnable_mean_parameters
from gdrf_amd.kernels import RBF
from gdrf_amd.optim import Adam

K, M, V, D = 3, 4, 5, 2
BASE_KEYS = {"_kernel.lengthscale_unconstrained", "_kernel.variance_unconstrained", "noise_unconstrained", "u_loc_unconstrained",
             "_word_topic_matrix_map_unconstrained", "u_scale_tril_unconstrained"}


class Trend(torch.nn.Module):
    """(K, n) linear trend in the inputs: weight (K, D) and bias (K, 1)."""

    def __init__(self, frozen_bias=False):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.arange(K * D, dtype=torch.float64).view(K, D) / 10)
        self.bias = torch.nn.Parameter(torch.ones(K, 1, dtype=torch.float64), requires_grad=not frozen_bias)

    def forward(self, x):
        return self.weight @ x.T + self.bias


class NoParams(torch.nn.Module):
    def forward(self, x):
        return x.sum(-1)


def host_model(mean_function):
    """A SparseMultinomialGDRF whose engine is a CPU stand-in: the layout a context with these sizes reports, laid out by hand."""
    named = learnable_mean_parameters(mean_function)
    eng = Engine.__new__(Engine)
    eng.K, eng.M, eng.V, eng.D, eng.ard, eng.kernel, eng.learn_inducing, eng.product = K, M, V, D, False, "rbf", False, None
    o_phi = 4 + K * M
    o_s = o_phi + K * V
    o_mean = o_s + K * M * M
    eng.mean_shapes = {n: p.shape for n, p in named}
    eng.mean_count = sum(p.numel() for _, p in named)
    eng.table = param_table(K, M, V, D, "rbf", mean_shapes=eng.mean_shapes, raw=dict(param=(0, 1, 2, 4, o_phi, o_s, o_mean + eng.mean_count),
                                                                                    mean=(o_mean, eng.mean_count)))
    total = o_mean + eng.mean_count
    eng.params, eng.grads = torch.arange(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    eng.exp_avg, eng.exp_avg_sq = torch.full((total,), 0.5, dtype=torch.float64), torch.full((total,), 0.25, dtype=torch.float64)
    eng.opt_step = 7
    model = SparseMultinomialGDRF.__new__(SparseMultinomialGDRF)
    model._engine, model._mean_function, model._mean_params = eng, mean_function, named
    model._mean_from_module()
    return model


def test_which_callables_are_learnable():
    assert learnable_mean_parameters(None) == []
    assert learnable_mean_parameters(lambda x: x.sum(-1)) == []
    assert learnable_mean_parameters(NoParams()) == []
    frozen = Trend()
    frozen.requires_grad_(False)
    assert learnable_mean_parameters(frozen) == []
    t = Trend()
    assert [n for n, _ in learnable_mean_parameters(t)] == ["_mean_function.weight", "_mean_function.bias"]
    assert learnable_mean_parameters(t)[0][1] is t.weight
    # a partly frozen module: only the trainable parameters form the segment
    assert [n for n, _ in learnable_mean_parameters(Trend(frozen_bias=True))] == ["_mean_function.weight"]


def test_state_dict_and_parameters_carry_the_mean_names():
    t = Trend()
    model = host_model(t)
    sd = model.state_dict()
    assert set(sd) == BASE_KEYS | {"_mean_function.weight", "_mean_function.bias"}
    assert torch.equal(sd["_mean_function.weight"], t.weight.detach()) and torch.equal(sd["_mean_function.bias"], t.bias.detach())
    assert len(model.parameters()) == 8
    assert host_model(lambda x: x.sum(-1)).state_dict().keys() == BASE_KEYS
    assert host_model(NoParams()).state_dict().keys() == BASE_KEYS


def test_optimizer_state_carries_the_mean_names():
    t = Trend()
    model = host_model(t)
    opt = Adam({"lr": 0.1})
    opt._bind(model._engine)
    st = opt.get_state()
    assert {"_mean_function.weight", "_mean_function.bias"} <= set(st)
    assert st["_mean_function.weight"]["exp_avg"].shape == (K, D) and st["_mean_function.weight"]["step"] == 7
    st["_mean_function.bias"]["exp_avg"] = torch.full((K, 1), 3.0)
    st["_mean_function.bias"]["exp_avg_sq"] = torch.full((K, 1), 4.0)
    opt.set_state(st)
    eng = model._engine
    assert torch.equal(eng.view("_mean_function.bias", eng.exp_avg), torch.full((K, 1), 3.0, dtype=torch.float64))
    assert torch.equal(eng.view("_mean_function.bias", eng.exp_avg_sq), torch.full((K, 1), 4.0, dtype=torch.float64))


def test_load_state_dict_writes_the_module_and_keeps_strict_semantics():
    t = Trend()
    model = host_model(t)
    sd = model.state_dict()
    sd["_mean_function.weight"] = torch.full((K, D), -2.0, dtype=torch.float64)
    assert model.load_state_dict(sd) == []
    assert torch.equal(t.weight.detach(), sd["_mean_function.weight"])                 # the module holds the loaded values
    assert torch.equal(model._engine.view("_mean_function.weight"), sd["_mean_function.weight"])
    # missing mean keys: strict raises, non-strict reports them and leaves the values
    base = {k: v for k, v in sd.items() if not k.startswith(MEAN_PREFIX)}
    with pytest.raises(RuntimeError, match="missing keys"):
        model.load_state_dict(base)
    assert set(model.load_state_dict(base, strict=False)) == {"_mean_function.weight", "_mean_function.bias"}
    assert torch.equal(t.weight.detach(), sd["_mean_function.weight"])
    # mean keys the model does not have: strict raises, non-strict ignores them
    plain = host_model(lambda x: x.sum(-1))
    with pytest.raises(RuntimeError, match="unexpected keys"):
        plain.load_state_dict(sd)
    assert plain.load_state_dict(sd, strict=False) == []
    # a wrong shape
    bad = dict(sd, **{"_mean_function.bias": torch.zeros(K, 2, dtype=torch.float64)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        model.load_state_dict(bad)


def test_module_writes_between_steps_reach_the_segment():
    t = Trend()
    model = host_model(t)
    assert model._mean_versions == [p._version for _, p in model._mean_params]
    with torch.no_grad():
        t.weight.fill_(5.0)
    assert model._mean_versions != [p._version for _, p in model._mean_params]     # _step_means reloads the segment then
    model._mean_from_module()
    assert torch.equal(model._engine.view("_mean_function.weight"), torch.full((K, D), 5.0, dtype=torch.float64))


def test_mean_parameters_on_another_device_raise():
    t = Trend()                                          # on the CPU; the model lives on a HIP device
    with pytest.raises(ValueError, match="device"):
        SparseMultinomialGDRF(num_observation_categories=V, num_topic_categories=K, world=[(0.0, 1.0)] * D,
                              kernel=RBF(input_dim=D), dirichlet_param=0.1, n_points=2, mean_function=t, device="cuda:0")
