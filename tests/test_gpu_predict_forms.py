"""GPU: every kernel form of the predictive mean path (gdrf_predict modes 0-4; predict() in csrc/api.hip) at its edges, form by form.

Five routes serve modes 0-3: 1 predict_mfma (K <= 32, LDS <= 64 KiB; DD in {2, GDRF_DMAX} x NB in {1, 2} x ARD, an rbf64 branch unrolled by
four with a clamped tail and a generic branch), 2 predict_rows with the coefficients in LDS, 3 predict_rows reading them from memory,
4 predict_rows_bigk (K > 32), 5 the streamed route.  Engine.last_forms() reports which one ran ("predict", "predict_nb"), and every case
asserts the form it targets, so a later change to a threshold fails the case instead of silently emptying it.  The cases, their inputs, the
plain numpy restatement they are compared with and the bound of each live in tests/_predict_ref.py (CPU only; its measures are tested by
tests/test_predict_forms_host.py).

Every call goes to eng.lib.gdrf_predict directly, as Engine.predict does, and writes into the interior of a larger buffer pre-filled with
NaN, 64 guard elements on either side (the interior stays 16-byte aligned): afterwards every interior element is finite and compared,
every guard element is still NaN.  Mode 3 is checked the same way on out_d, and its out_d[1] equals sum w exactly.  Within one route the
result of rows [:n1] is bit-identical to the first n1 rows of the full call (modes 0-2, n1 no multiple of 16).

A case passes when relerr(device, exact) <= 64 e_ref + floor (tests/_predict_ref.py; mode 3 by the perplexity of its two sums).  Largest
measured / allowed ratio per route on an MI355X, with the case that gives it:

  route                                 case                  mode       n   measured      e_ref      bound  ratio
  1 predict_mfma, NB = 1                mfma-D1-ard-rbf       0         37   2.01e-14   1.11e-14   8.11e-13  0.025
  1 predict_mfma, NB = 2                mfma-pure-K17         3         65   6.82e-08   2.64e-08   1.69e-06  0.040
  2 predict_rows, coefficients in LDS   rows-lds-f32          3        129   3.43e-07   6.12e-09   3.92e-07  0.876
  3 predict_rows, from memory           rows-mem-pure         3        129   5.99e-07   2.84e-08   1.81e-06  0.330
  4 predict_rows_bigk                   bigk-K33-f32          0        129   3.18e-08   3.18e-08   2.15e-06  0.015
  5 streamed                            streamed-K40-V70-f32  3        131   1.55e-07   5.70e-09   3.65e-07  0.425
  mode 4 (step forward + predict_var)   locvar-unwhitened     4 var    257   1.37e-13   1.01e-13   6.56e-12  0.021

Every case of every route stays under its bound; no bound had to be reasoned about beyond the formula.  The closest one, route 2 in the
GDRF_F32 context at mode 3 (V = 1413), is the float32 normaliser of Phi: build_phi_kernel adds the V exponentials of a topic one after
another in the array precision, numpy's float32 sum in the restatement adds them pairwise, and a relative error of the normaliser shifts
every log p of that topic alike, so it reaches the perplexity undamped (3.4e-7 is three float32 ulps; the same term gives routes 3 and 5
their largest ratios).  Everything in float64, and modes 0-2 everywhere, sits at 1-4 % of the bound.
"""

import numpy as np
import pytest
import torch

from tests import _predict_ref as R

pytestmark = pytest.mark.gpu

if not R.HAS_LONGDOUBLE:
    pytest.skip("np.longdouble has no more precision than float64 here: the exact restatement needs eps < 1e-18", allow_module_level=True)

GUARD = 64
FORM_NAME = {1: "mfma", 2: "rows_lds", 3: "rows_mem", 4: "rows_bigk", 5: "streamed"}


def _engine(g, inp):
    from gdrf_amd.engine import Engine
    dtype = torch.float64 if g["ctx"] == "f64" else torch.float32
    eng = Engine(g["n_cap"] or 64, g["M"], g["K"], g["V"], g["D"], dtype=dtype, kernel=g["kind"], jitter=inp["jitter"], process_group=None,
                 pure_fp32=g["ctx"] == "pure", whiten=g["whiten"], ard=g["ard"], rows_form="streamed" if g["streamed"] else "auto")
    t = lambda a: torch.as_tensor(np.asarray(a)).to(eng.device, dtype)
    eng.set_inducing_points(t(inp["Z"]))
    eng.set_dirichlet(torch.full((g["K"], g["V"]), 0.01))
    eng.view("log_lengthscale").copy_(t(inp["log_ls"]).reshape(eng.view("log_lengthscale").shape))
    eng.view("log_variance").copy_(t(inp["log_var"]))
    eng.view("u_loc").copy_(t(inp["u"]))
    eng.view("phi_unc").copy_(t(inp["phi_unc"]))
    if g["kind"] == "rationalquadratic":
        eng.view("log_scale_mixture").copy_(t(inp["log_alpha"]))
    if g["mode4"]:
        eng.view("u_scale_tril_unc").copy_(t(inp["S_unc"]))
    # the engine holds exactly the reference's numbers: float32-valued inputs in the float32 context types
    assert np.array_equal(eng.view("u_loc").cpu().double().numpy(), inp["u"]) and np.array_equal(eng.Z.cpu().double().numpy(), inp["Z"])
    assert eng.factorize() == 0
    return eng


def _guarded(shape, dtype, device):
    """A NaN-filled buffer with GUARD elements on either side of an interior of `shape`; (buffer, interior view)."""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), float("nan"), dtype=dtype, device=device)
    assert (buf.data_ptr() + GUARD * buf.element_size()) % 16 == 0
    return buf, buf[GUARD:GUARD + size].view(shape)


def _predict(eng, g, X, ws, n, mode):
    """gdrf_predict(mode) on the leading n rows into guarded buffers; the interior as a tensor (mode 3: the two doubles of out_d)."""
    from gdrf_amd import _lib
    from gdrf_amd.engine import _stream_ptr
    K, V = g["K"], g["V"]
    shape = {0: (K, n), 1: (n, K), 2: (n, V), 3: None, 4: (2, K, n)}[mode]
    dbuf, dint = _guarded((2,), torch.float64, eng.device)
    obuf, oint = _guarded(shape, eng.dtype, eng.device) if shape else (None, None)
    wptr = None
    if mode == 3:
        wptr = eng._counts_ptr(ws) if g["csr"] else ws.data_ptr()
    _lib.check(eng.lib.gdrf_predict(eng.ctx, X.data_ptr(), n, eng.Z.data_ptr(), eng.params.data_ptr(), wptr, mode,
                                    oint.data_ptr() if shape else None, dint.data_ptr(), _stream_ptr(eng.device)), "gdrf_predict")
    torch.cuda.synchronize(eng.device)
    for buf, interior, used in ((obuf, oint, shape is not None), (dbuf, dint, mode == 3)):
        if buf is None:
            continue
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), (g["id"], mode, n, "a guard element was written")
        if used:
            assert bool(torch.isfinite(interior).all()), (g["id"], mode, n, "an interior element was left at its sentinel or is not finite")
        else:
            assert bool(torch.isnan(interior).all()), (g["id"], mode, n, "an output this mode does not own was written")
    return dint if mode == 3 else oint


def _check(g, mode, n, got, key=None):
    e, b = R.measure(got, R.exact_output(g, mode, n, key)), R.bound(g, mode, n, key)
    print("%-32s form %s n %6d mode %d %-5s err %.2e  e_ref %.2e  bound %.2e  ratio %.3f"
          % (g["id"], g["form"], n, mode, key or "", e, b[0], b[1], e / b[1]))
    assert b[1] <= R.CEILING[g["ctx"]]
    return e <= b[1], (g["id"], mode, n, key, e, b)


@pytest.mark.parametrize("gid", [g["id"] for g in R.GROUPS])
def test_predictive_form(gid):
    g = R.BY_ID[gid]
    inp, _, _ = R.reference(gid)
    eng = _engine(g, inp)
    dtype = eng.dtype
    X = torch.as_tensor(inp["X"]).to(eng.device, dtype).contiguous()
    assert np.array_equal(X.cpu().double().numpy(), inp["X"])
    ws = torch.as_tensor(inp["ws"]).to(eng.device).contiguous()
    failures = []
    for n in g["ns"]:
        if g["csr"]:
            from gdrf_amd.data import to_csr
            ws_n = to_csr(ws[:n])
        else:
            ws_n = ws
        for mode in g["modes"]:
            out = _predict(eng, g, X, ws_n, n, mode)
            forms = eng.last_forms()
            if mode == 4:          # the step's forward: the predictive slots stay as they were (unset in a fresh context)
                assert "predict" not in forms and "predict_nb" not in forms, forms
                o = out.cpu().numpy()
                failures += [_check(g, 4, n, o[0], "loc4"), _check(g, 4, n, o[1], "var")]
                continue
            assert forms.get("predict") == FORM_NAME[g["form"][0]] and forms.get("predict_nb", 0) == g["form"][1], (gid, mode, n, forms)
            if mode == 3:
                s = out.cpu().numpy()
                assert s[1] == float(inp["ws"][:n].astype(np.int64).sum()), (gid, n, s)
                failures.append(_check(g, 3, n, R.perplexity(s[0], s[1])))
            else:
                failures.append(_check(g, mode, n, out.cpu().numpy()))
    # row independence: the leading n1 rows alone give the same bits as the leading n1 rows of the largest call
    n1, nmax = g["n1"], max(g["ns"])
    if n1 is not None:
        assert n1 % 16 and n1 < nmax
        for mode in (m for m in g["modes"] if m <= 2):
            full, part = _predict(eng, g, X, ws, nmax, mode), _predict(eng, g, X, ws, n1, mode)
            assert torch.equal(full[:, :n1] if mode == 0 else full[:n1], part), (gid, mode, "rows [:n1] differ from the full call's")
    bad = [f[1] for f in failures if not f[0]]
    assert not bad, bad
