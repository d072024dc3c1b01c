"""CPU tests of the optimizer surface (gdrf_amd.optim): the pyro.optim registry of gdrf/train_script.py:73-87, torch's argument
names and defaults, clip_args and per-parameter callables, and the state format before an engine is bound."""
import pytest

NEW = {"adamax": dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
       "rmsprop": dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False),
       "adagrad": dict(lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10),
       "adadelta": dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0),
       "asgd": dict(lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0.0),
       "rprop": dict(lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50.0)),
       "adagradrmsprop": dict(eta=1.0, delta=1e-16, t=0.1)}


@pytest.mark.parametrize("name", sorted(NEW))
def test_new_optimizers_construct_with_torch_defaults(name):
    from gdrf_amd.optim import OPTIMIZER_DICT
    o = OPTIMIZER_DICT[name]()
    assert o.args == NEW[name] and o.segmented
    assert type(o).__name__.lower() == name
    key = "eta" if name == "adagradrmsprop" else "lr"
    o = OPTIMIZER_DICT[name]({key: 0.5})
    assert o.lr == 0.5 and o.args[key] == 0.5


@pytest.mark.parametrize("name", sorted(NEW) + ["adam", "adamw", "clippedadam"])
@pytest.mark.parametrize("bad", ["nonsense", "foreach", "capturable", "differentiable", "fused", "maximize"])
def test_unknown_and_unsupported_torch_arguments_raise(name, bad):
    from gdrf_amd.optim import OPTIMIZER_DICT
    with pytest.raises(ValueError):
        OPTIMIZER_DICT[name]({bad: False})


def test_adagradrmsprop_has_no_lr():
    from gdrf_amd.optim import AdagradRMSProp
    with pytest.raises(ValueError):
        AdagradRMSProp({"lr": 1e-3})


@pytest.mark.parametrize("name", ["sgd", "sparseadam", "dctadam"])
def test_remaining_registry_entries_still_raise(name):
    from gdrf_amd.optim import OPTIMIZER_DICT
    with pytest.raises(NotImplementedError):
        OPTIMIZER_DICT[name]({"lr": 0.1})


def test_clip_args_validation():
    from gdrf_amd.optim import Adam, RMSprop
    assert not Adam({"lr": 0.1}).segmented
    o = Adam({"lr": 0.1}, clip_args={"clip_norm": 2.0, "clip_value": 0.5})
    assert o.segmented and o.clip_for("u_loc") == {"clip_norm": 2.0, "clip_value": 0.5}
    assert not Adam({"lr": 0.1}, clip_args={}).segmented
    assert RMSprop(clip_args={"clip_value": 1}).clip_for("phi_unc") == {"clip_value": 1.0}
    with pytest.raises(ValueError):
        Adam(clip_args={"max_norm": 1.0})
    with pytest.raises(ValueError):
        Adam(clip_args={"clip_norm": -1.0})
    with pytest.raises(TypeError):
        Adam(clip_args=[1.0])


def test_callable_arguments_get_param_store_names():
    from gdrf_amd.optim import RMSprop, param_store_name
    assert param_store_name("u_loc") == "u_loc"
    assert param_store_name("log_lengthscale") == "_kernel.lengthscale"
    assert param_store_name("phi_unc") == "_word_topic_matrix_map"
    assert param_store_name("u_scale_tril_unc") == "u_scale_tril"
    assert param_store_name("_mean_function.w") == "_mean_function.w"
    seen = []

    def args(module_name, param_name):
        seen.append((module_name, param_name))
        return {"lr": 0.5} if param_name == "u_loc" else {"momentum": 0.9}

    def clip(module_name, param_name):
        return {"clip_norm": 1.0} if param_name == "_kernel.lengthscale" else {}

    o = RMSprop(args, clip_args=clip)
    assert o.segmented
    assert o.args_for("u_loc")["lr"] == 0.5 and o.args_for("u_loc")["momentum"] == 0.0
    assert o.args_for("log_variance")["momentum"] == 0.9 and o.args_for("log_variance")["lr"] == 1e-2
    o.args_for("u_loc")
    assert seen == [("u_loc", "u_loc"), ("_kernel.variance", "_kernel.variance")]      # asked once per parameter
    assert o.clip_for("log_lengthscale") == {"clip_norm": 1.0} and o.clip_for("u_loc") == {}
    with pytest.raises(ValueError):
        RMSprop(lambda m, p: {"maximize": True}).args_for("u_loc")
    with pytest.raises(TypeError):
        RMSprop(lambda m, p: 0.1).args_for("u_loc")
    with pytest.raises(ValueError):
        RMSprop(clip_args=lambda m, p: {"norm": 1.0}).clip_for("u_loc")


@pytest.mark.parametrize("name", sorted(NEW))
def test_state_before_binding_is_kept_for_the_engine(name):
    import torch
    from gdrf_amd.optim import OPTIMIZER_DICT
    o = OPTIMIZER_DICT[name]()
    assert o.get_state() == {}
    st = {"u_loc": {"step": 3, "lr": 0.25, "sum": torch.ones(2, 3)}}
    o.set_state(st)
    assert o.get_state() is st
