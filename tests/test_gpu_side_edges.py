"""GPU sweep of the two side paths of a training step at every form edge and option: the custom-link step (gdrf_step_local_link:
rows_vstream_kernel<T, VS_LINK, 8 | 32>, rows_csr_kernel<T, VS_LINK, LG, KJ> with csr_link_const_kernel, rows_mu_kernel, rows_sites_kernel)
and the two-point step of a non-unit world (gdrf_step_local2: elbo_rows2_sites_kernel and the sequencing of two backwards around swapped
row adjoints).  The cases, their data and the references are those of tests/_side_ref.py; tests/test_side_edges_host.py shows on the CPU
that they cross the edges they name and that the clamp cases would catch a normaliser that forgot the clamp.

One step per case, then
  - the loss and every gradient block against RefShapedGDRF.loss_and_grads (autograd) at the same jitter level;
  - the row workspaces q, mu, vbar, locbar and (two-point) g_locbar against the row reference (autograd with respect to the predictive);
  - fp64: LOSS_TOL_VS_TORCH for the loss, 1e-7 per block, TOL[float64]["w"] for q and mu and 10 x that for the adjoints;
  - float32: TOL[float32]["loss"]; tensor blocks, the three scalar hyper-parameters as ONE block (tests/test_gpu_round3.py::_scalar_block)
    and any further scalar block held to max(TOL[float32]["g"], 6 x max|mu| 2^-24), the resolution float32 leaves for the link's argument;
  - CSR cases: the counts go in as the CSR tensor, and the result also equals the dense step's to 1e-12 in fp64.
Every measured error is printed (pytest -s).

Measured on one MI355X (largest over the cases of a path and dtype; loss | worst gradient block | worst row output):
see DESIGN.md, "Testing notes of the side paths"."""
import gc

import numpy as np
import pytest
import torch

from tests import _side_ref as R
from tests._util import LOSS_TOL_VS_TORCH, dev, engine_for
from tests.test_gpu_parity import TOL
from tests.test_gpu_round3 import _scalar_block

pytestmark = pytest.mark.gpu

DTYPE = {"fp64": torch.float64, "fp32": torch.float32}
SCALARS = ("log_lengthscale", "log_variance", "log_noise")


def _counts(m, eng, csr):
    if not csr:
        return dev(m.ws, eng, torch.int32)
    from gdrf_amd.data import to_csr
    return to_csr(m.ws.to(torch.int32).to(eng.device))


def _step(c, m, eps, csr, level=None):
    """one step of the engine on the case; (engine, loss, {block: gradient})"""
    eng = engine_for(m, dtype=DTYPE[c["regime"]], n_cap=c["n_cap"], device="cuda:0", mfma_mode=c["mfma_mode"], store_t=c["store_t"],
                     hyper_backward=c["hyper_backward"])
    kw = {}
    xs_m = m.scale(m.xs)
    if c["path"] == "link":
        eng.link_function = R._LINKS[c["link"]]
    else:
        xs_g = m.scale(xs_m)
        kw.update(xs_guide=dev(xs_g, eng))
        if c["mean"]:
            kw.update(mean=dev(R.MEAN_FN(xs_m), eng), mean_guide=dev(R.MEAN_FN(xs_g), eng))
    if level is not None:
        kw["force_level"] = level
    if c["renyi"] is not None:
        kw["renyi_alpha"] = c["renyi"]
    eng.loss_and_grads(dev(xs_m, eng), _counts(m, eng, csr), dev(eps, eng), **kw)
    out = eng.read_out()
    assert out["chol_failed"] == 0
    return eng, out["loss"], {name: v.cpu().double().numpy().copy() for name, v in eng.named_views(eng.grads).items()}


def _err(got, ref, floor=0.0):
    """(max |got - ref| less the floors of round-off that is neither side's error, max |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return max(float((np.abs(got - ref) - floor).max()) - R.ABS_FLOOR, 0.0), float(np.abs(ref).max())


def _rel(got, ref, floor=0.0):
    e, r = _err(got, ref, floor)
    return e / max(r, 1e-300)


def _check(cid):
    c = R.CASES[cid]
    m, eps, _ = R.build(c)
    two, fp32, csr = c["path"] == "two", c["regime"] == "fp32", c["route"] == "csr"
    level = None
    if two:      # the level is the oracle's, forced on the engine (tests/test_gpu_round2.py)
        loss_ref, g_ref = R.oracle_loss_and_grads(m, c, eps)
        level = m.last_jitter_level
    eng, loss, grads = _step(c, m, eps, csr, level)
    if not two:  # the level is the engine's, forced on the oracle
        level = eng.last_jitter_level
        loss_ref, g_ref = R.oracle_loss_and_grads(m, c, eps, level)
    if fp32 and c["clamp_word"] is not None:
        loss_ref += R.eps32_loss_shift(m, c)
    if c["forms"]:
        forms = eng.last_forms()
        assert {k: forms.get(k) for k in c["forms"]} == c["forms"], forms
    if c["hyper_backward"] == "tn":
        assert eng.hyper_backward == "tn"
    if c["mfma_mode"] != "auto":
        assert eng.mfma_mode == c["mfma_mode"]
    if c["store_t"] is True:
        assert eng.stores_t
    n = m.N
    rows = {name: eng.workspace(name, n).cpu().double().numpy() for name in ("q", "mu", "vbar", "locbar") + (("g_locbar",) if two else ())}
    ref = R.row_reference(m, eps[-1] if eps.dim() == 3 else eps, level)          # the workspaces hold the last particle's rows

    # the link path's cancellation floor (tests/_side_ref.py::link_cancellation_floor) on what thetabar - cn rowsum reaches directly
    floors = {}
    if not two:
        fl = R.link_cancellation_floor(m, ref, c["V"], float(torch.finfo(DTYPE[c["regime"]]).eps)).numpy()
        e_last = (eps[-1] if eps.dim() == 3 else eps).numpy()
        floors = dict(locbar=fl, vbar=fl * np.abs(e_last), u_loc=fl @ np.abs(ref["W_m"].numpy()) / n)
    t = TOL[DTYPE[c["regime"]]]
    rep = {"loss": abs(loss - loss_ref) / abs(loss_ref)}
    assert set(grads) == set(g_ref), (set(grads), set(g_ref))
    eabs, refs = {}, {}
    for name in grads:
        eabs[name], refs[name] = _err(grads[name], g_ref[name].numpy().reshape(grads[name].shape), floors.get(name, 0.0) if c["particles"] == 1 else 0.0)
        rep["g_" + name] = eabs[name] / max(refs[name], 1e-300)
    for name in rows:
        rep[name] = _rel(rows[name], ref[name].numpy(), floors.get(name, 0.0))
    mu_res = float(np.abs(rows["mu"]).max()) * 2.0 ** -24
    if fp32:
        rep["g_hyper_scalars"] = _scalar_block(eabs, refs)
        rep["mu_resolution"] = mu_res
    print("SIDE", c["path"], c["regime"], cid, "level", level, {k: f"{v:.2e}" for k, v in rep.items()})

    for name in ("q", "mu"):
        assert rep[name] < t["w"], (name, rep)
    for name in ("vbar", "locbar") + (("g_locbar",) if two else ()):
        assert rep[name] < 10 * t["w"], (name, rep)
    if fp32:
        assert rep["loss"] < t["loss"], rep
        tol = max(t["g"], 6.0 * mu_res)
        for name in grads:
            if name not in SCALARS:
                assert rep["g_" + name] < tol, (name, tol, rep)
        assert rep["g_hyper_scalars"] < tol, (tol, rep)
    else:
        assert rep["loss"] <= LOSS_TOL_VS_TORCH, rep
        for name in grads:
            assert rep["g_" + name] < 1e-7, (name, rep)
        if not two:      # rows with no counts: cn = 0 and thetabar = 0, so the link's Jacobian sees exact zeros
            empty = (m.ws.sum(1) == 0).numpy()
            assert empty.sum() >= 3 and np.abs(rows["locbar"][:, empty]).max() == 0.0
    if (c["K"], c["V"]) == (1, 2) and c["clamp_word"] is not None:
        assert np.abs(rows["locbar"]).max() == 0.0 and np.abs(grads["u_loc"]).max() == 0.0      # both words clamped: no likelihood gradient
    del eng
    if csr and not fp32:
        # the same step on the dense counts
        eng_d, loss_d, grads_d = _step(c, m, eps, False, level)
        assert abs(loss - loss_d) <= 1e-12 * abs(loss_d), (loss, loss_d)
        for name in grads:
            assert _rel(grads[name], grads_d[name]) <= 1e-12, name
        del eng_d
    gc.collect()


@pytest.mark.parametrize("cid", [c["id"] for c in R.LINK_CASES])
def test_link_step(cid):
    _check(cid)


@pytest.mark.parametrize("cid", [c["id"] for c in R.TWO_CASES])
def test_two_point_step(cid):
    _check(cid)


def test_link_function_with_xs_guide_is_still_refused():
    c = R.CASES["two-K9-V32-fp64"]
    m, eps, _ = R.build(c)
    eng = engine_for(m, device="cuda:0")
    eng.link_function = R._LINKS["sigmoid"]
    xs_m = m.scale(m.xs)
    with pytest.raises(NotImplementedError):
        eng.loss_and_grads(dev(xs_m, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), xs_guide=dev(m.scale(xs_m), eng), force_level=0)


def test_two_point_step_refuses_a_context_that_stores_t():
    """gdrf_step_local2 runs its two backwards on the dense W-bar form; a store_t=True context is refused on the host, before any launch"""
    from gdrf_amd import _lib
    c = dict(R.CASES["two-fp32-f32"], store_t=True, mfma_mode="auto")
    m, eps, _ = R.build(c)
    with pytest.raises(_lib.GdrfHipError, match="needs the dense Wbar form"):
        _step(c, m, eps, False, 0)
