"""The solve side of a step at every tile edge: K_nm in the solve precision (knm_rbf_f64_kernel, knm_kernel<TS, T, false>), W = K_nm L^-T with
its row norms q (gemm_nt<FwdWProb>, TRI == 1) and the backward through K_nm (gemm_nt<BwdKnmProb>, TRI == 2, in its LDS-transposed and generic
epilogues, the LZ / ARD / PER variants, and the hyper-TN alternative), each against the long-double product of the engine's OWN buffers under
a derived bound.  The cases, their data, the references and the bounds are those of tests/_solve_ref.py; tests/test_solve_edges_host.py shows
on the CPU that the table crosses every edge it names and that these measures see each simulated fault at 10x its bound.

One forced-level step per case, then, with every got / bound ratio printed (pytest -s) and required to stay below 1:
  K_nm     workspace Knm against the direct form, elementwise and per 128 x 64 tile;
  W        workspace W against Knm_got Linv_got^T, elementwise and per 128 x 64 tile;
  q        workspace q against the row sums of the stored W^2, and against those of (Knm_got Linv_got^T)^2;
  red_d    [4], [5], [6] against sum (Wbar_got Linv_got) o {K, dK/dlog ls, dK/dlog alpha}; G[j][d] (learn_inducing), the per-coordinate and
           per-period tails (ARD, Periodic, Product) behind it; hyper_backward="tn": [4] and [5] at the split arithmetic's bound;
  G^T      red_T's block against W_got^T Wbar_got.
Also: the padded columns M .. Mp-1 of the flat Knm and W buffers are exactly zero in every row below n, LinvT is the exact transpose of Linv,
the forms are the ones the case names, and a second identical step is bit-identical in W, q and red_d[4 ..].

Measured on one MI355X: see DESIGN.md, "Testing notes of the solve side"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _solve_ref as R
from tests._util import dev

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]
if not R.HAS_LONGDOUBLE:
    pytest.skip("numpy's longdouble is no wider than float64 here", allow_module_level=True)


def _engine(name):
    from gdrf_amd.engine import Engine
    c, d = R.CASES[name], R.inputs(name)
    dtype = torch.float64 if c["ctx"] == "f64" else torch.float32
    o = c["opts"]
    kw = dict(dtype=dtype, kernel=c["kind"], jitter=R.JITTER, process_group=None, pure_fp32=c["ctx"] == "pure",
              learn_inducing=bool(o.get("learn_inducing")), ard=bool(o.get("ard")), mfma_mode=o.get("mfma_mode", "auto"),
              hyper_backward="tn" if o.get("hyper_tn") else "auto")
    if c["kind"] == "product":
        kw["product"] = R.PRODUCT_TABLE
    eng = Engine(c["n_cap"], c["M"], c["K"], c["V"], c["D"], **kw)
    eng.set_inducing_points(torch.from_numpy(d["Z"]))
    eng.set_dirichlet(torch.ones(c["K"], c["V"], dtype=torch.float64))
    for pname, v in d["params"].items():
        view = eng.view(pname)
        view.copy_(torch.as_tensor(np.asarray(v), dtype=torch.float64).to(dtype).reshape(view.shape))
    return eng, c, d


def _flat(eng, name):
    """The whole padded buffer of a workspace, by a direct gdrf_ws_copy."""
    from gdrf_amd import _lib
    from gdrf_amd.engine import _WS_IDS, _stream_ptr
    ptr, cnt = C.c_void_p(), C.c_int64()
    _lib.check(eng.lib.gdrf_ws_ptr(eng.ctx, _WS_IDS[name], C.byref(ptr), C.byref(cnt)), "gdrf_ws_ptr")
    esz = eng.lib.gdrf_ws_elem_size(eng.ctx, _WS_IDS[name])
    flat = torch.empty(cnt.value, dtype=torch.float32 if esz == 4 else torch.float64, device=eng.device)
    _lib.check(eng.lib.gdrf_ws_copy(eng.ctx, _WS_IDS[name], flat.data_ptr(), cnt.value, _stream_ptr(eng.device)), "gdrf_ws_copy")
    torch.cuda.synchronize(eng.device)
    return flat.cpu().numpy()


def _step(eng, c, d):
    n = c["n"]
    X = dev(d["X"], eng)
    eng.loss_and_grads(X, dev(d["ws"], eng, torch.int32), dev(d["eps"], eng), force_level=R.LEVEL)
    assert eng.read_out()["chol_failed"] == 0
    r = {k: eng.workspace(k, n).cpu().double().numpy() for k in ("Knm", "W", "q", "Wbar", "Linv", "LinvT")}
    r["X"], r["Z"] = X.cpu().double().numpy(), eng.Z.cpu().double().numpy()
    r["params"] = {k: eng.view(k).cpu().double().numpy() for k in d["params"]}
    r["red_d"] = eng.red_d.cpu().numpy().copy()
    r["red_T"] = eng.red_T.cpu().double().numpy()
    r["W_flat"], r["Knm_flat"] = _flat(eng, "W"), _flat(eng, "Knm")
    return r


@pytest.mark.parametrize("name", list(R.CASES))
def test_solve_side_against_long_double_products_of_the_engine_buffers(name):
    eng, c, d = _engine(name)
    f = R.facts(c)
    M, n, Mp, Dk = c["M"], c["n"], f["Mp"], f["D"]
    got = _step(eng, c, d)
    forms = eng.last_forms()
    tn = bool(c["opts"].get("hyper_tn"))
    assert forms.get("hyper") == ("tn" if tn else "f64"), (name, forms)
    assert eng.pure_fp32 == (c["ctx"] == "pure") and eng.last_jitter_level == R.LEVEL
    if c["ctx"] == "f32":
        assert eng.mfma_mode == c["opts"].get("mfma_mode", "f16x3"), eng.mfma_mode

    ratios = {}
    # K_nm
    kn = R.knm(c, got["X"], got["Z"], got["params"])
    ratios["Knm"] = R.ratio(got["Knm"], kn["k"], kn["bound"])
    ratios["Knm_tile"] = R.tile_ratio(got["Knm"], kn["k"], kn["bound"])
    # W and q
    W, Wb = R.w_ref(c, got["Knm"], got["Linv"])
    ratios["W"] = R.ratio(got["W"], W, Wb)
    ratios["W_tile"] = R.tile_ratio(got["W"], W, Wb)
    q, qb, q2, qb2 = R.q_ref(c, got["W"], W, Wb)
    ratios["q"] = R.ratio(got["q"], q, qb)
    ratios["q_acc"] = R.ratio(got["q"], q2, qb2)
    # the backward sums
    Kb, Kbb = R.kbar_ref(c, got["Wbar"], got["Linv"])
    T, P = R.terms(c, kn, got["Knm"])
    val, bnd = R.sums(c, Kb, Kbb, T, P)
    red = got["red_d"]
    per_axis = bool(c["opts"].get("ard")) or R.sources(c) is not None
    if tn:
        b4, b5 = R.tn_bounds(c, got["Wbar"], got["W"], Wb, T, got["Linv"])
        ratios["s1_tn"] = R.ratio(red[4], val["s1"], b4)
        ratios["s2_tn"] = R.ratio(red[5], val["s2"], b5)
    else:
        ratios["s1"] = R.ratio(red[4], val["s1"], bnd["s1"])
        if not per_axis:                                   # ARD and periodic contexts split the lengthscale sum by coordinate
            ratios["s2"] = R.ratio(red[5], val["s2"], bnd["s2"])
    if c["kind"] == "rationalquadratic":
        ratios["s3"] = R.ratio(red[6], val["s3"], bnd["s3"])
        assert red[6] != 0
    else:
        assert red[6] == 0, (name, red[6])
    if c["opts"].get("learn_inducing"):
        ratios["G"] = R.ratio(red[8:8 + M * Dk].reshape(M, Dk), val["G"], bnd["G"])
    if per_axis:
        tail = red[8 + M * Dk:]
        ratios["axis"] = R.ratio(tail[:Dk], val["axis"], bnd["axis"])
        if "period" in val:
            npair = val["period"].shape[0]
            ratios["period"] = R.ratio(tail[Dk:Dk + npair], val["period"], bnd["period"])
    # G^T
    lay = eng.red_layout
    GT, GTb = R.gt_ref(c, got["W"], got["Wbar"])
    ratios["GT"] = R.ratio(got["red_T"][lay["GT"]:lay["GT"] + Mp * Mp].reshape(Mp, Mp)[:M, :M], GT, GTb)

    shares = R.no_negligible_tile(c, W, Kb, T)
    print(name, forms)
    print("   ratios", {k: "%.3g" % v for k, v in ratios.items()})
    print("   smallest tile shares", {k: "%.1e" % v for k, v in shares.items()})

    # the padding: columns M .. Mp-1 of every row below n are exactly zero
    for buf in ("Knm_flat", "W_flat"):
        pad = got[buf].reshape(c["n_cap"], Mp)[:n, M:]
        assert not pad.any(), (name, buf, float(np.abs(pad).max()))
    assert np.array_equal(got["LinvT"], got["Linv"].T), name
    assert np.array_equal(np.tril(got["Linv"]), got["Linv"]), name
    # a second identical step: bit-identical (fixed accumulation order)
    again = _step(eng, c, d)
    end = lay["mean"]
    for k in ("W_flat", "q"):
        assert np.array_equal(got[k], again[k]), (name, k)
    assert np.array_equal(red[4:end], again["red_d"][4:end]), (name, np.flatnonzero(red[4:end] != again["red_d"][4:end])[:8])
    bad = {k: v for k, v in ratios.items() if not v < 1.0}
    assert not bad, (name, bad)
