"""CPU tests of the fold-in surface (csrc/foldin.h): the library exports its entry point, the header and the ctypes signature agree, the
methods exist, and the argument errors are raised before any device call (a model cannot be built without a HIP device, so its methods
are called on a stub that has nothing an engine or a device would need)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("infer_topic_probs", "infer_log_topic_probs", "topic_counts", "completion_perplexity")


def stub(link=None):
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Stub:
        K, _K, V, _V, _link_function = 3, 3, 5, 5, link
        _fold_in = G._fold_in
    return Stub()


def call(name, s, xs, ws, ws_score=None, **kw):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    if name == "completion_perplexity":
        return G.completion_perplexity(s, xs, ws, ws if ws_score is None else ws_score, **kw)
    return getattr(G, name)(s, xs, ws, **kw)


def test_library_exports_the_entry_point(hip_lib):
    from gdrf_amd import _lib
    assert hasattr(hip_lib, "gdrf_fold_in")
    res, args = _lib.SIGNATURES["gdrf_fold_in"]
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    decl = re.search(r"\bint gdrf_fold_in\(([^;]*)\);", header)
    assert decl and decl.group(1).startswith("gdrf_ctx* ctx, const void* X_dev, int64_t n,")
    params = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(args) == 20
    # ctx, X, n, Z, params | ws, crow, col, val | ws2, crow2, col2, val2 | mode, num_iters, tol | out, diag, out_d, stream
    import ctypes as C
    for p, a in zip(params, args):
        want = C.c_int64 if p.startswith("int64_t ") else C.c_int if p.startswith("int ") else C.c_double if p.startswith("double ") else C.c_void_p
        assert a is want, (p, a)
    for name in ("GDRF_FI_THETA = 0", "GDRF_FI_MU = 1", "GDRF_FI_COUNTS = 2", "GDRF_FI_SCORE = 3"):
        assert name in header


def test_the_methods_exist_on_the_model_on_a_snapshot_and_on_the_engine():
    from gdrf_amd.engine import Engine, check_fold_args
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        for name in METHODS:
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Engine.fold_in) and callable(check_fold_args)


@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("kw,match", [(dict(num_iters=-1), "num_iters"), (dict(num_iters=2.5), "num_iters"), (dict(tol=-1e-3), "tol"),
                                      (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol")])
def test_bad_num_iters_and_tol_are_value_errors(name, kw, match):
    xs, ws = torch.rand(4, 2), torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match=match):
        call(name, stub(), xs, ws, **kw)


@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("shape", [(4, 4), (3, 5), (4, 5, 1), (20,)])
def test_counts_of_another_shape_are_a_value_error(name, shape):
    with pytest.raises(ValueError, match="ws"):
        call(name, stub(), torch.rand(4, 2), torch.ones(shape, dtype=torch.int32))


def test_a_w_score_of_another_shape_or_sparsity_is_a_value_error():
    from gdrf_amd.data import to_csr
    xs, ws = torch.rand(4, 2), torch.ones(4, 5, dtype=torch.int32)
    for bad in (torch.ones(4, 4, dtype=torch.int32), torch.ones(3, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="ws_score"):
            call("completion_perplexity", stub(), xs, ws, bad)
    with pytest.raises(ValueError, match="sparse"):
        call("completion_perplexity", stub(), xs, ws, to_csr(ws))
    with pytest.raises(ValueError, match="sparse"):
        call("completion_perplexity", stub(), xs, to_csr(ws), ws)
    with pytest.raises(ValueError, match="ws_score"):
        call("completion_perplexity", stub(), xs, to_csr(ws), to_csr(torch.ones(4, 4, dtype=torch.int32)))
    from gdrf_amd.models import SparseMultinomialGDRF as G
    with pytest.raises(ValueError, match="w_score"):
        G.completion_perplexity(stub(), xs, ws, None)


def test_the_engine_raises_before_the_device_too():
    from gdrf_amd.data import to_csr
    from gdrf_amd.engine import Engine
    xs, ws = torch.rand(4, 2), torch.ones(4, 5, dtype=torch.int32)
    s = stub()
    with pytest.raises(ValueError, match="mode"):
        Engine.fold_in(s, xs, ws, 4)
    with pytest.raises(ValueError, match="num_iters"):
        Engine.fold_in(s, xs, ws, 0, num_iters=-2)
    with pytest.raises(ValueError, match="tol"):
        Engine.fold_in(s, xs, ws, 0, tol=float("nan"))
    with pytest.raises(ValueError, match="ws"):
        Engine.fold_in(s, xs, ws[:, :4], 0)
    with pytest.raises(ValueError, match="sparse"):
        Engine.fold_in(s, xs, ws, 3, ws_score=to_csr(ws))
    with pytest.raises(ValueError, match="mode 3"):
        Engine.fold_in(s, xs, ws, 0, ws_score=ws)


@pytest.mark.parametrize("name", METHODS)
def test_a_custom_link_is_not_implemented(name):
    xs, ws = torch.rand(4, 2), torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="link_function"):
        call(name, stub(link=staticmethod(lambda mu: torch.softmax(mu, -2))), xs, ws)
