"""CPU tests of the sparse (CSR) count input (csrc/rows_csr.h): the library exports its binding call, gdrf_amd.data cuts CSR tensors by rows,
and a malformed count matrix is rejected by a plain function - and by the model constructor - before the GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_csr_binding(hip_lib):
    from gdrf_amd import _lib
    assert "gdrf_bind_counts_csr" in _lib.SIGNATURES and hasattr(hip_lib, "gdrf_bind_counts_csr")
    header = open(os.path.join(ROOT, "include", "gdrf_hip.h")).read()
    assert re.search(r"\bint gdrf_bind_counts_csr\(gdrf_ctx\* ctx, const int64_t\* crow_dev", header)
    res, args = _lib.SIGNATURES["gdrf_bind_counts_csr"]
    assert len(args) == 8            # ctx, crow, col, val, n, nnz, ccol, cperm


def test_sparse_is_a_keyword_of_train_and_the_helpers_exist():
    from gdrf_amd import data
    from gdrf_amd.train import train
    assert inspect.signature(train).parameters["sparse"].default is False
    for name in ("to_csr", "csr_rows", "check_counts"):
        assert callable(getattr(data, name))


def _dense(n=23, V=17, seed=0, density=0.3):
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 9, size=(n, V)).astype(np.int32)
    d[rng.random((n, V)) > density] = 0
    d[[2, 3, n - 1]] = 0                     # empty rows, the last one included
    return d


def test_to_csr_round_trips():
    from gdrf_amd.data import to_csr
    d = _dense()
    for src in (d, torch.from_numpy(d), torch.from_numpy(d).long()):
        c = to_csr(src)
        assert c.layout == torch.sparse_csr and c.values().dtype == torch.int32 and c.crow_indices().dtype == torch.int64
        assert np.array_equal(c.to_dense().numpy(), d)
    with pytest.raises(ValueError, match="2-d"):
        to_csr(np.zeros(5, dtype=np.int32))


@pytest.mark.parametrize("sel", [slice(0, 10), slice(5, None), slice(None), slice(7, 7), slice(None, None, 2), slice(20, 400),
                                 np.array([4, 4, 0, 22, 3, 4]), np.array([], dtype=np.int64), [1], 6, np.array([-1, -23]),
                                 torch.tensor([5, 2, 2])])
def test_csr_rows_equals_dense_slicing(sel):
    from gdrf_amd.data import csr_rows, to_csr
    d = _dense()
    c = to_csr(d)
    got = csr_rows(c, sel)
    idx = sel.numpy() if isinstance(sel, torch.Tensor) else sel
    want = d[idx] if isinstance(idx, slice) else d[np.atleast_1d(np.asarray(idx, dtype=np.int64))]
    assert got.layout == torch.sparse_csr and got.values().dtype == torch.int32 and tuple(got.shape) == want.shape
    assert int(got.crow_indices()[0]) == 0 and int(got.crow_indices()[-1]) == got.values().numel()
    assert np.array_equal(got.to_dense().numpy(), want)
    # a cut of a cut, and the source is left as it was
    again = csr_rows(got, slice(0, 1))
    assert np.array_equal(again.to_dense().numpy(), want[:1])
    assert np.array_equal(c.to_dense().numpy(), d)


def test_csr_rows_rejects_bad_input():
    from gdrf_amd.data import csr_rows, to_csr
    c = to_csr(_dense())
    with pytest.raises(IndexError):
        csr_rows(c, np.array([0, 23]))
    with pytest.raises(ValueError, match="sparse_csr"):
        csr_rows(c.to_dense(), slice(0, 2))


def _raw(crow, col, val, size, idt=torch.int64, vdt=torch.int32):
    return torch.sparse_csr_tensor(torch.tensor(crow, dtype=idt), torch.tensor(col, dtype=idt), torch.tensor(val, dtype=vdt), size=size)


GOOD = dict(crow=[0, 2, 2, 3], col=[4, 0, 1], val=[1, 2, 3], size=(3, 5))


def test_check_counts_accepts_well_formed_matrices():
    from gdrf_amd.data import check_counts, to_csr
    check_counts(torch.zeros(3, 5, dtype=torch.int32), 3, 5, "cpu")
    check_counts(_raw(**GOOD), 3, 5, "cpu")
    check_counts(_raw(**GOOD, idt=torch.int32), 3, 5)
    check_counts(to_csr(_dense()), 23, 17)
    check_counts(_raw([0, 0], [], [], (1, 5)), 1, 5)          # no entries at all


BAD = [
    ("dtype", lambda: _raw(**GOOD, vdt=torch.int64)),
    ("dtype", lambda: _raw(**GOOD, vdt=torch.float32)),
    ("shape", lambda: _raw(GOOD["crow"], GOOD["col"], GOOD["val"], (3, 6))),
    ("shape", lambda: _raw([0, 2, 2, 3, 3], GOOD["col"], GOOD["val"], (4, 5))),
    ("crow_indices", lambda: _raw([1, 2, 2, 3], GOOD["col"], GOOD["val"], (3, 5))),
    ("crow_indices", lambda: _raw([0, 2, 2, 2], GOOD["col"], GOOD["val"], (3, 5))),
    ("crow_indices", lambda: _raw([0, 2, 1, 3], GOOD["col"], GOOD["val"], (3, 5))),
    ("col_indices", lambda: _raw(GOOD["crow"], [4, 0, 5], GOOD["val"], (3, 5))),
    ("col_indices", lambda: _raw(GOOD["crow"], [4, -1, 1], GOOD["val"], (3, 5))),
    ("layout", lambda: _raw(**GOOD).to_sparse_coo()),
    ("layout", lambda: _raw(**GOOD).to_sparse_csc()),
]


@pytest.mark.parametrize("prop,make", BAD)
def test_check_counts_names_the_offending_property(prop, make):
    from gdrf_amd.data import check_counts
    with pytest.raises(ValueError, match=prop):
        check_counts(make(), 3, 5)


def test_check_counts_names_the_device():
    from gdrf_amd.data import check_counts
    with pytest.raises(ValueError, match="device"):
        check_counts(_raw(**GOOD), 3, 5, "cuda:0")
    with pytest.raises(ValueError, match="dtype"):
        check_counts(torch.zeros(3, 5, dtype=torch.int64), 3, 5)


def test_engine_validation_calls_check_counts():
    """Engine._chk_rows hands a sparse ws to check_counts (an Engine cannot be built without a HIP device, so it is called unbound)"""
    from gdrf_amd.engine import Engine

    class Stub:
        device, dtype, D, V = torch.device("cpu"), torch.float32, 2, 5
    xs = torch.zeros(3, 2)
    Engine._chk_rows(Stub, xs, _raw(**GOOD))
    Engine._chk_rows(Stub, xs, torch.zeros(3, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="col_indices"):
        Engine._chk_rows(Stub, xs, _raw(GOOD["crow"], [4, 0, 5], GOOD["val"], (3, 5)))
    with pytest.raises(ValueError, match="shape"):
        Engine._chk_rows(Stub, torch.zeros(4, 2), _raw(**GOOD))


@pytest.mark.parametrize("prop,make", [b for b in BAD if b[0] != "shape"] + [("shape", lambda: _raw(GOOD["crow"], GOOD["col"], GOOD["val"], (3, 6)))])
def test_model_rejects_a_malformed_csr_matrix_before_touching_the_gpu(prop, make):
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    with pytest.raises(ValueError, match=prop):
        SparseMultinomialGDRF(xs=torch.rand(3, 2), ws=make(), world=[(0.0, 1.0)] * 2,
                              kernel=RBF(input_dim=2, lengthscale=torch.tensor(0.2), variance=torch.tensor(1.0)),
                              num_observation_categories=5, num_topic_categories=2, dirichlet_param=0.01, n_points=[2, 2],
                              device="cpu")


def test_what_csr_rows_cuts_from_a_checked_matrix_counts_as_checked():
    from gdrf_amd.data import check_counts, csr_rows
    c = _raw(**GOOD)
    from gdrf_amd.data import csr_to, is_checked, mark_checked
    assert not is_checked(csr_rows(c, slice(0, 2)))
    check_counts(c, 3, 5)
    part = csr_rows(c, np.array([2, 0]))
    assert is_checked(part) and is_checked(csr_to(part, "cpu"))
    check_counts(part, 2, 5)
    # a matrix declared well formed skips the index checks (that is the declaration's meaning), one that is not does not
    bad = _raw(GOOD["crow"], [4, 0, 5], GOOD["val"], (3, 5))
    with pytest.raises(ValueError, match="col_indices"):
        check_counts(bad, 3, 5)
    check_counts(mark_checked(_raw(**GOOD)), 3, 5)
