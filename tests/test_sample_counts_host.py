"""CPU tests of the count-sampling surface (csrc/sample_counts.h): the library exports its entry point, the header and the ctypes
signature agree, the methods exist, and the argument errors are raised before any device call (a model cannot be built without a HIP
device, so its methods are called on a stub that has nothing an engine or a device would need)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, V, N, S = 3, 5, 4, 2


def stub(V=V):
    """What the methods read before they reach the device; anything else (an engine, _prepare_inputs) is an AttributeError"""
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Stub:
        _link_function = None
        _count_args = G._count_args
    Stub.K = Stub._K = K
    Stub.V = Stub._V = V
    Stub.M = 6
    return Stub()


def sample(s, xs=None, totals=10, num_samples=S, **kw):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    return G.sample_counts(s, torch.rand(N, 2) if xs is None else xs, totals, num_samples, **kw)


def check(s, ws, xs=None, **kw):
    from gdrf_amd.models import SparseMultinomialGDRF as G
    return G.predictive_check(s, torch.rand(N, 2) if xs is None else xs, ws, **kw)


def test_library_exports_the_entry_point(hip_lib):
    from gdrf_amd import _lib
    from gdrf_amd.engine import SAMPLE_COUNTS_MAX_V
    assert hasattr(hip_lib, "gdrf_sample_counts")
    res, args = _lib.SIGNATURES["gdrf_sample_counts"]
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    decl = re.search(r"\bint gdrf_sample_counts\(([^;]*)\);", header)
    assert decl and decl.group(1).startswith("gdrf_ctx* ctx, const void* theta_dev, int64_t n,")
    params = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    # ctx, theta, n, params, totals, tmax, ws | mode, num_samples, seed, row_offset | u, out, dev, zeros, stream
    assert len(params) == len(args) == 16 and res is C.c_int
    for p, a in zip(params, args):
        want = (C.c_int64 if p.startswith("int64_t ") else C.c_uint64 if p.startswith("uint64_t ") else C.c_int if p.startswith("int ")
                else C.c_void_p)
        assert a is want, (p, a)
    for name in ("GDRF_SC_COUNTS = 0", "GDRF_SC_STATS = 1", "GDRF_SC_UNIFORMS = 2"):
        assert name in header
    limit = re.search(r"#define GDRF_SC_MAX_V (\d+)", header)
    assert limit and int(limit.group(1)) == SAMPLE_COUNTS_MAX_V >= 4096


def test_the_methods_exist_on_the_model_on_a_snapshot_and_on_the_engine():
    from gdrf_amd.engine import Engine, check_count_args
    from gdrf_amd.models.sparse_gdrf import ModelSnapshot, SparseMultinomialGDRF
    for cls in (SparseMultinomialGDRF, ModelSnapshot):
        for name in ("sample_counts", "predictive_check"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(Engine.sample_counts) and callable(Engine.fill_token_uniforms) and callable(check_count_args)


@pytest.mark.parametrize("kw,match", [
    (dict(num_samples=0), "num_samples"), (dict(num_samples=-3), "num_samples"), (dict(num_samples=2.5), "num_samples"),
    (dict(totals=-1), "totals"), (dict(totals=torch.tensor([3, 2, -1, 4])), "totals"), (dict(totals=torch.tensor([3, 2, 1])), "totals"),
    (dict(totals=torch.tensor([3.0, 2.0, 1.0, 4.0])), "totals"), (dict(totals=torch.ones(N, 1, dtype=torch.int64)), "totals"),
    (dict(theta=torch.rand(S, N, K + 1)), "theta"), (dict(theta=torch.rand(S + 1, N, K)), "theta"), (dict(theta=torch.rand(S, K, N)), "theta"),
    (dict(u=torch.rand(S, N, 9, dtype=torch.float64)), "too few tokens"), (dict(u=torch.rand(S, N + 1, 10, dtype=torch.float64)), "u must"),
    (dict(u=torch.rand(S, N, 10)), "float64"), (dict(u=torch.full((S, N, 10), 1.0, dtype=torch.float64)), r"\[0, 1\)"),
    (dict(u=torch.full((S, N, 10), -1e-9, dtype=torch.float64)), r"\[0, 1\)"),
    (dict(u=torch.full((S, N, 10), float("nan"), dtype=torch.float64)), r"\[0, 1\)"),
])
def test_bad_sample_counts_arguments_are_value_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        sample(stub(), **kw)


def test_a_vocabulary_above_the_limit_is_a_value_error_that_states_the_limit():
    from gdrf_amd.engine import SAMPLE_COUNTS_MAX_V
    big = stub(V=SAMPLE_COUNTS_MAX_V + 1)
    with pytest.raises(ValueError, match=str(SAMPLE_COUNTS_MAX_V)):
        sample(big)
    with pytest.raises(ValueError, match=str(SAMPLE_COUNTS_MAX_V)):
        check(big, torch.ones(N, SAMPLE_COUNTS_MAX_V + 1, dtype=torch.int32))


def test_coherent_samples_take_at_most_the_joint_row_limit():
    from gdrf_amd.engine import JOINT_MAX_ROWS
    with pytest.raises(ValueError, match="JOINT_MAX_ROWS"):
        sample(stub(), xs=torch.rand(JOINT_MAX_ROWS + 1, 2), coherent=True)


def test_bad_predictive_check_arguments_are_value_errors():
    from gdrf_amd.data import to_csr
    ws = torch.ones(N, V, dtype=torch.int32)
    with pytest.raises(ValueError, match="sparse"):
        check(stub(), to_csr(ws))
    for bad in (ws[:, :4], ws[:3], ws.reshape(-1), ws.double()):
        with pytest.raises(ValueError, match="ws"):
            check(stub(), bad)
    with pytest.raises(ValueError, match="num_samples"):
        check(stub(), ws, num_samples=0)


def test_the_engine_raises_before_the_device_too():
    from gdrf_amd.data import to_csr
    from gdrf_amd.engine import Engine, SAMPLE_COUNTS_MAX_V, check_count_args
    s = stub()
    th, tot, ws = torch.rand(S, N, K), torch.full((N,), 10, dtype=torch.int32), torch.ones(N, V, dtype=torch.int32)
    assert check_count_args(th, tot, K, V) == (S, N, 10)
    assert check_count_args(th, tot, K, V, 1, ws, torch.rand(S, N, 12, dtype=torch.float64)) == (S, N, 10)
    for kw, match in [(dict(mode=2), "mode"), (dict(mode=1), "ws"), (dict(ws=ws), "mode 1"), (dict(mode=1, ws=to_csr(ws)), "sparse"),
                      (dict(mode=1, ws=ws[:, :4]), "ws"), (dict(row_offset=-1), "row_offset"),
                      (dict(u=torch.rand(S, N, 9, dtype=torch.float64)), "too few tokens"),
                      (dict(u=torch.full((S, N, 10), 1.0, dtype=torch.float64)), r"\[0, 1\)")]:
        with pytest.raises(ValueError, match=match):
            Engine.sample_counts(s, th, tot, **kw)
    with pytest.raises(ValueError, match="totals"):
        Engine.sample_counts(s, th, tot - 11)
    with pytest.raises(ValueError, match="totals"):
        Engine.sample_counts(s, th, tot[:3])
    with pytest.raises(ValueError, match="theta"):
        Engine.sample_counts(s, th[:, :, :2], tot)
    with pytest.raises(ValueError, match="theta"):
        Engine.sample_counts(s, th[0], tot)
    with pytest.raises(ValueError, match=str(SAMPLE_COUNTS_MAX_V)):
        Engine.sample_counts(stub(V=SAMPLE_COUNTS_MAX_V + 1), th, tot)
    with pytest.raises(ValueError, match="fill_token_uniforms"):
        Engine.fill_token_uniforms(s, 1, 0, 0, N, 10)
    with pytest.raises(ValueError, match="fill_token_uniforms"):
        Engine.fill_token_uniforms(s, 1, 2, -1, N, 10)
