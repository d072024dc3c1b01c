"""CPU: the measure tests/test_gpu_predict_forms.py holds the predictive path to (tests/_predict_ref.py).  The exact restatement agrees
with the reference-shaped oracle, the bound computed from the two restatements stays under the suite's ceiling at every listed shape, and
each simulated kernel fault lands at least 100 x above the bound of the case it is applied to."""
import numpy as np
import pytest
import torch

from tests import _predict_ref as R

if not R.HAS_LONGDOUBLE:
    pytest.skip("np.longdouble has no more precision than float64 here: the exact restatement needs eps < 1e-18", allow_module_level=True)

LD = R.LD


@pytest.mark.parametrize("gid", ["mfma-rows-f64", "bigk-K33-V11"])
def test_exact_restatement_agrees_with_the_oracle(gid):
    from oracle.gdrf_oracle import RefShapedGDRF
    g = R.BY_ID[gid]
    n = max(g["ns"])
    inp, exact, _ = R.reference(gid)
    m = RefShapedGDRF(inp["X"], inp["ws"], kind=g["kind"], K=g["K"], lengthscale=float(np.exp(inp["log_ls"])), variance=25.0,
                      jitter=inp["jitter"], Z=torch.from_numpy(inp["Z"]), force_jitter_level=0, dtype=torch.float64)
    with torch.no_grad():
        m.params["log_lengthscale"].copy_(torch.tensor(float(inp["log_ls"]), dtype=torch.float64))
        m.params["log_variance"].copy_(torch.tensor(float(inp["log_var"]), dtype=torch.float64))
        m.params["u_loc"].copy_(torch.from_numpy(inp["u"]))
        m.params["phi_unc"].copy_(torch.from_numpy(inp["phi_unc"]))
    got = {0: m.log_topic_probs().numpy(), 1: m.topic_probs().numpy(), 2: m.word_probs().numpy(), 3: float(m.perplexity())}
    for mode in (0, 1, 2, 3):
        e, b = R.relerr(got[mode], R.exact_output(g, mode, n)), R.bound(g, mode, n)[1]
        print(f"{gid} mode {mode}: oracle vs exact {e:.2e}, bound {b:.2e}")
        assert e <= b, (gid, mode, e, b)


def test_the_computed_bound_stays_under_the_ceiling_at_every_listed_shape():
    worst = {}
    for g in R.GROUPS:
        for n in g["ns"]:
            for mode in g["modes"]:
                for key in R.MODE_KEYS.get(mode, (None,)):
                    e, b = R.bound(g, mode, n, key)
                    assert np.isfinite(b) and b <= R.CEILING[g["ctx"]], (g["id"], mode, n, key, e, b)
                    worst[g["ctx"]] = max(worst.get(g["ctx"], 0.0), b)
    print({c: f"{b:.2e} (ceiling {R.CEILING[c]:.0e})" for c, b in worst.items()})


def test_every_group_takes_the_route_it_is_named_for():
    want = {"mfma": 1, "rows-lds": 2, "rows-mem": 3, "bigk": 4, "streamed": 5, "csr": 5, "locvar": 1}
    for g in R.GROUPS:
        prefix = next(p for p in sorted(want, key=len, reverse=True) if g["id"].startswith(p))
        assert g["form"][0] == want[prefix], (g["id"], g["form"])
    assert {g["form"] for g in R.GROUPS} >= {(1, 1), (1, 2), (2, 0), (3, 0), (4, 0), (5, 0)}
    ts = {c: np.dtype(R.CTX[c][0]).itemsize for c in R.CTX}
    for c in ("f64", "pure"):          # the LDS conditions the issue states for routes 2 and 3, per solve-precision element size
        g2, g3 = R.BY_ID[f"rows-lds-{c}"], R.BY_ID[f"rows-mem-{c}"]
        for g in (g2, g3):
            assert R.lds_bytes(1, g["M"], g["D"], g["K"], g["V"], ts[c]) > R.LDS_FORM
        assert R.lds_bytes(2, g2["M"], g2["D"], g2["K"], g2["V"], ts[c]) <= R.LDS_FORM
        assert R.lds_bytes(2, g3["M"], g3["D"], g3["K"], g3["V"], ts[c]) > R.LDS_FORM >= 0
        assert R.lds_bytes(3, g3["M"], g3["D"], g3["K"], g3["V"], ts[c]) <= R.LDS_MAX
    assert R.BY_ID["rows-lds-pure"]["V"] != R.BY_ID["rows-lds-f64"]["V"]
    assert R.LONG_MFMA > R.GRID_ROWS_MFMA and R.LONG_ROWS > R.GRID_ROWS


def _seen(name, got, g, mode, n):
    m, b = R.measure(got, R.exact_output(g, mode, n)), R.bound(g, mode, n)[1]
    print("%-58s measure %.2e  bound %.2e" % (name, m, b))
    assert m >= 100 * b, (name, m, b)


def test_the_measure_sees_each_simulated_fault():
    # the last 16-row group left at its sentinel (n = 253: rows 240 .. 252)
    g = R.BY_ID["mfma-rows-f64"]
    for mode in (0, 1, 2):
        out = np.array(R.exact_output(g, mode, 253), dtype=np.float64)
        if mode == 0:
            out[:, 240:] = np.nan
        else:
            out[240:] = np.nan
        _seen(f"mode {mode}: last 16-row group left at its sentinel", out, g, mode, 253)
    # the last inducing point dropped from the sum, at an M with a tail (M = 13: M4 = 16, four steps, the rbf64 loop's clamped tail)
    for gid in ("mfma-M13-rbf", "mfma-M5-matern32"):
        g = R.BY_ID[gid]
        _, exact, _ = R.reference(gid)
        loc = exact["loc"] - (exact["Knm"][:, -1:] @ exact["Cf"][:, -1:].T).T
        _seen(f"{gid} mode 0: last inducing point dropped", loc, g, 0, 37)
        _seen(f"{gid} mode 1: last inducing point dropped", R.softmax(loc, 0).T, g, 1, 37)
    # topics 0-15 and 16-31 swapped (the two column blocks of NB = 2)
    g = R.BY_ID["mfma-K32"]
    perm = np.r_[16:32, 0:16]
    _seen("mode 0: 16-topic blocks swapped", R.exact_output(g, 0, 37)[perm], g, 0, 37)
    _seen("mode 1: 16-topic blocks swapped", R.exact_output(g, 1, 37)[:, perm], g, 1, 37)
    p = R.exact_output(g, 1, 37)[:, perm] @ R.softmax(R.reference("mfma-K32")[0]["phi_unc"].astype(LD), 1)
    _seen("mode 2: 16-topic blocks swapped", p, g, 2, 37)
    # the rows of one wave written with the float C/D row map (row 4 (lane >> 4) + r) in place of the double one ((lane >> 4) + 4 r)
    g = R.BY_ID["mfma-rows-f64"]
    wrong = np.arange(16).reshape(4, 4).T.flatten()          # the row that lands where row i belongs
    for mode in (0, 1, 2):
        out = np.array(R.exact_output(g, mode, 64))
        if mode == 0:
            out[:, 16:32] = out[:, 16 + wrong]
        else:
            out[16:32] = out[16 + wrong]
        _seen(f"mode {mode}: one wave's rows in the float row map", out, g, mode, 64)
    # one row of a second grid-stride pass written twice and its neighbour not at all
    for gid, first in (("mfma-long", R.GRID_ROWS_MFMA), ("rows-lds-long", R.GRID_ROWS), ("bigk-long", R.GRID_ROWS)):
        g = R.BY_ID[gid]
        n = max(g["ns"])
        for mode in (0, 1):
            out = np.array(R.exact_output(g, mode, n))
            if mode == 0:
                out[:, first + 6] = out[:, first + 5]
            else:
                out[first + 6] = out[first + 5]
            _seen(f"{gid} mode {mode}: a second-pass row written twice", out, g, mode, n)
    # one count row left out of sum w: the count itself is held exactly, the perplexity to its bound
    for gid, n in (("mfma-rows-f64", 253), ("mfma-rows-f32", 65), ("mfma-long", R.LONG_MFMA)):
        g = R.BY_ID[gid]
        inp, exact, _ = R.reference(gid)
        s0, s1 = R.perp_sums(exact["logp"][:n], inp["ws"][:n])
        row = n - 1
        s1_less = s1 - int(inp["ws"][row].sum())
        assert inp["ws"][row].sum() > 0 and s1_less != s1            # seen by the exact comparison of out_d[1] at any n
        if n < 1000:                                                 # and by the perplexity where one row is not a 1e-5 share of the sum
            _seen(f"{gid} mode 3: one count row left out of sum w", R.perplexity(s0, s1_less), g, 3, n)
    # and the exact result passes
    g = R.BY_ID["mfma-rows-f64"]
    for mode in (0, 1, 2, 3):
        assert R.measure(R.exact_output(g, mode, 253), R.exact_output(g, mode, 253)) == 0
