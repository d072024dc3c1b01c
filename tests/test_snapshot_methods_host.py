"""CPU tests of the model methods a ModelSnapshot forwards to the device model it rebuilds (SNAPSHOT_METHODS of
gdrf_amd/models/sparse_gdrf.py): every name is a real function on the class with the model method's signature and docstring, and a call
hands its positional and keyword arguments to the same method of ``restore()`` unchanged."""
import inspect

import pytest

from gdrf_amd.models.sparse_gdrf import SNAPSHOT_METHODS, ModelSnapshot, SparseMultinomialGDRF


def test_the_table_names_each_public_predictive_method_once():
    assert len(set(SNAPSHOT_METHODS)) == len(SNAPSHOT_METHODS) == 27
    for name in SNAPSHOT_METHODS:
        assert not name.startswith("_") and inspect.isfunction(vars(SparseMultinomialGDRF)[name]), name


@pytest.mark.parametrize("name", SNAPSHOT_METHODS)
def test_a_snapshot_method_has_the_signature_and_the_docstring_of_the_models(name):
    mine, model = vars(ModelSnapshot)[name], vars(SparseMultinomialGDRF)[name]
    assert inspect.isfunction(mine) and mine is not model
    a, b = inspect.signature(mine).parameters, inspect.signature(model).parameters
    assert list(a) == list(b) and list(a)[0] == "self"
    assert [(p.kind, p.default) for p in a.values()] == [(p.kind, p.default) for p in b.values()]
    assert mine.__doc__ is model.__doc__ and mine.__name__ == name and mine.__qualname__ == f"ModelSnapshot.{name}"


@pytest.mark.parametrize("name", SNAPSHOT_METHODS)
def test_a_snapshot_method_forwards_positionals_and_keywords_unchanged(name):
    calls, args, kwargs = [], (object(), object()), dict(seed=object(), anything=object())

    class Model:
        pass

    def method(self, *a, **kw):
        calls.append((self, a, kw))
        return "result"
    setattr(Model, name, method)
    model = Model()

    class Snap:
        def restore(self):
            return model
    assert getattr(ModelSnapshot, name)(Snap(), *args, **kwargs) == "result"
    assert getattr(ModelSnapshot, name)(Snap()) == "result"
    assert len(calls) == 2 and calls[0][0] is model and calls[0][1] == args and calls[0][2] == kwargs
    assert all(x is y for x, y in zip(calls[0][1], args)) and all(calls[0][2][k] is v for k, v in kwargs.items())
    assert calls[1][1:] == ((), {})


def test_what_a_snapshot_answers_itself_stays_its_own():
    for name in ("dims", "K", "V", "word_topic_matrix"):
        assert isinstance(vars(ModelSnapshot)[name], property), name
    for name in ("restore", "half", "float", "state_dict", "parameters", "to_payload", "__getstate__", "__setstate__"):
        assert name not in SNAPSHOT_METHODS and inspect.isfunction(vars(ModelSnapshot)[name]), name
