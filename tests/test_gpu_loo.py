"""GPU tests of PSIS leave-one-out (gdrf_predict_loo and gdrf_psis_rows, csrc/predict_loo.h) against the float64 restatement of
tests/_loo_ref.py.

The stage kernel is fed float64 matrices built on the CPU, so its arithmetic is checked on exact inputs: pareto_k within 1e-8
absolute, elpd_loo within 1e-10 of the row's largest |a|, ess within 1e-8 relative, NaN exactly where the restatement has NaN
(_loo_ref.K_CAP, ELPD_CAP, ESS_CAP; they are caps - reordered double sums over at most 96 terms differ near 1e-13 - not measurements).

The fused kernel runs on the model and the counts of tests/test_gpu_predict_score.py (tests/_score_ref.py::counts with top = 200, the
last row empty) with injected eps.  Its log likelihoods are held to the predictive path's TOL against _score_ref.log_liks (V = 1: every
a_s is 0 in exact arithmetic, the error is taken over the largest row total as _score_ref.errors takes it); the PSIS maps are held to the
stage caps against the restatement applied to the DEVICE's log_lik, which keeps the float32 rounding of a_s - amplified about tenfold
into pareto_k - out of the check of the PSIS arithmetic.
"""
import math

import pytest
import torch

from gdrf_amd.data import csr_rows, to_csr
from gdrf_amd.engine import LOO_NAMES, loo_tail_len
from tests import _loo_ref as LR
from tests._mc_util import MEAN_KN, _model, build, engine
from tests._score_ref import TOL, counts, log_liks
from tests._util import dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
STAGE_S = (25, 26, 63, 64, 65, 257, 1024)                   # both sides of every power of two, and the two ends
ELPD, PK, ESS, LPD, TOT, COEF = range(6)


@pytest.fixture(scope="module")
def stage_engine():
    """any engine serves the stage: it reads no model quantity"""
    return engine(build(2, 8, torch.float64), torch.float64)


def pairs_row(S, g):
    """Gaussian values whose M + 1 largest importance ratios (the smallest a) are tied in pairs"""
    a = torch.randn(S, generator=g, dtype=torch.float64) - 20.0
    idx = a.argsort()[:LR.tail_len(S) + 1]
    a[idx[1::2]] = a[idx[0:2 * len(idx[1::2]):2]]
    return a


def degenerate_rows(S):
    """(S, 3): all values equal; all but four equal, the four below them; a tail whose lower quartile underflows"""
    a = torch.full((S, 3), -5.0, dtype=torch.float64)
    a[:4, 1] = torch.tensor([-9.0, -8.0, -7.0, -6.0], dtype=torch.float64)
    a[:, 2] = -400.0 * torch.arange(S, dtype=torch.float64)
    return a


def stage_matrix(S):
    """(a, first degenerate column): exact GPD tails, Gaussian a_s of three widths, the degenerate kinds, ties in the tail"""
    g = torch.Generator().manual_seed(S)
    cols = [LR.gpd_tail_rows(S, (-0.2, 0.0, 0.3, 0.7, 1.2)) - 50.0]
    for sd in (0.1, 1.0, 5.0):
        cols.append(sd * torch.randn(S, 4, generator=g, dtype=torch.float64) - 1000.0)
    n_deg = sum(c.shape[1] for c in cols)
    cols.append(degenerate_rows(S))
    cols.append(torch.stack([pairs_row(S, g), pairs_row(S, g)], 1))
    return torch.cat(cols, 1).contiguous(), n_deg


def same(x, y):
    """bit for bit, NaN where NaN"""
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))


def held(got, ref, a, what):
    figs = LR.errors(got, ref, a)
    print(what, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in figs.items()})
    assert LR.within_caps(figs), (what, figs)
    return figs


def test_names_match_the_reference_module():
    assert LOO_NAMES == LR.NAMES and all(loo_tail_len(S) == LR.tail_len(S) for S in range(25, 1025))


@pytest.mark.parametrize("S", STAGE_S)
def test_the_stage_on_exact_inputs(S, stage_engine):
    eng = stage_engine
    a, deg = stage_matrix(S)
    ref = LR.psis(a)
    got = eng.psis_rows(a.to(eng.device))
    assert got.shape == (3, a.shape[1]) and got.dtype == torch.float64
    held(got, ref, a, f"stage S={S}")
    nan = torch.isnan(got[PK]).cpu()
    assert bool(nan[deg:deg + 3].all()) and not bool(nan[:deg].any())          # the tied rows: as the restatement has them (M = 5: not fitted)
    assert S < 64 or not bool(nan[deg + 3:].any())
    assert abs(float(got[ELPD, deg]) + 5.0) < 1e-13 and abs(float(got[ESS, deg]) - S) < 1e-9 * S       # all equal: elpd_loo = a, ess = S
    RP, _, _, _, lds = LR.stage_plan(S)
    assert eng.last_loo_plan() == dict(RP=RP, lds=lds)
    zero = eng.psis_rows(torch.zeros(S, 3, dtype=torch.float64, device=eng.device))                   # an empty row
    assert torch.equal(zero[ELPD], torch.zeros_like(zero[ELPD])) and bool(torch.isnan(zero[PK]).all())


@pytest.mark.parametrize("S", [25, 1024])
def test_the_stage_at_every_row_count_round_a_workgroup_pass(S, stage_engine):
    """n = 1, RP - 1, RP, RP + 1 and, the grid being at most 1024 workgroups, 1024 RP + 6 rows: a workgroup takes two passes, the last
    partly filled.  A row's result does not depend on the call it is in."""
    eng = stage_engine
    RP = LR.stage_plan(S)[0]
    n = 1024 * RP + 6
    a = (torch.randn(S, n, generator=torch.Generator().manual_seed(S + 1), dtype=torch.float64) - 300.0).contiguous()
    ad = a.to(eng.device)
    big = eng.psis_rows(ad)
    ends = torch.cat([torch.arange(40), torch.arange(n - 40, n)])
    held(big[:, ends.to(eng.device)], LR.psis(a[:, ends]), a[:, ends], f"stage S={S} n={n} (two passes)")
    assert not bool(torch.isnan(big).any())
    for k in (1, RP - 1, RP, RP + 1):
        assert torch.equal(eng.psis_rows(ad[:, :k].contiguous()), big[:, :k]), k
    assert torch.equal(eng.psis_rows(ad[:, n - 7:].contiguous()), big[:, n - 7:])


# K, V, S, n: a sparse cross of both sides of every lane-group form, the chunk edges of the vocabulary and the ends and power-of-two
# sides of the sample range; K = 128, V = 129, S = 1024 in float64 is the largest launch (142504 bytes of LDS at RP = 1): it must fit
FUSED = [(1, 50, 25, 70), (8, 1, 64, 70), (9, 128, 257, 70), (17, 129, 64, 70), (33, 300, 25, 70), (65, 50, 64, 70), (128, 129, 1024, 24),
         (8, 300, 1024, 40), (128, 50, 257, 40)]


def fused_case(m, eng, ws, eps, S, mean=None, what=""):
    """checks (a) .. (d) and (f) of one model, counts and draws; returns the dense maps"""
    dtype, n, K, V = eng.dtype, ws.shape[0], eps.shape[1], ws.shape[1]
    a_ref = log_liks(m, m.xs[:n], ws, eps)
    xs, wd, ed = dev(m.xs[:n], eng), dev(ws, eng, torch.int32), dev(eps, eng)
    top = float(ws.sum(-1).max())
    outs = {}
    for form, w in (("dense", wd), ("csr", to_csr(wd))):
        out, a = eng.predict_loo(xs, w, S, eps=ed, mean=mean, return_log_lik=True)
        assert out.shape == (6, n) and a.shape == (S, n) and out.dtype == a.dtype == torch.float64
        plan = LR.loo_plan(K, V, S, 8 if dtype == torch.float64 else 4, LR.lane_group(K), form == "csr")
        assert eng.last_loo_plan() == dict(RP=plan[0], lds=plan[4]), (form, plan)
        # (a) the log likelihoods
        err = float((a.cpu() - a_ref).abs().max()) / (top if V == 1 else float(a_ref.abs().max()))
        print(f"{what} {form} log_lik {err:.2e}")
        assert err < TOL[dtype], (form, err)
        # (b) the PSIS maps against the restatement on the device's own log_lik; lpd from the same values
        held(out[:3], LR.psis(a.cpu()), a, f"{what} {form} fused")
        lpd = torch.logsumexp(a, 0) - math.log(S)
        assert float((out[LPD] - lpd).abs().max()) <= 1e-12 * max(1.0, float(lpd.abs().max()))
        assert torch.equal(out[TOT].cpu(), ws.double().sum(-1))
        # (c) the stage kernel on the same values
        held(eng.psis_rows(a), out[:3], a, f"{what} {form} stage vs fused")
        # (d) lpd, total and log_coef are predict_score's, bit for bit
        score = eng.predict_score(xs, w, S, eps=ed, mean=mean)
        assert torch.equal(out[LPD], score[0]) and torch.equal(out[TOT], score[3]) and torch.equal(out[COEF], score[4]), form
        # without the matrix: the same maps
        assert same(eng.predict_loo(xs, w, S, eps=ed, mean=mean), out), form
        outs[form] = out
    # (f) the two forms add a row's words in different orders
    d, c = outs["dense"], outs["csr"]
    assert float((d[ELPD] - c[ELPD]).abs().max()) / (top if V == 1 else float(d[ELPD].abs().max())) < TOL[dtype]
    assert torch.equal(torch.isnan(d[PK]), torch.isnan(c[PK]))
    # the empty last row: elpd_loo = 0, nothing fitted, every draw weighs the same
    assert float(d[ELPD, -1]) == 0.0 == float(c[ELPD, -1]) and bool(torch.isnan(d[PK, -1])) and abs(float(d[ESS, -1]) - S) < 1e-9 * S
    assert bool(torch.isnan(d[PK])[d[TOT] == 0].all())         # so is every row without a token
    if K == 1:                                               # theta = 1: constant a_s, no row is fitted
        assert bool(torch.isnan(d[PK]).all())
    return d


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,V,S,n", FUSED)
def test_the_fused_kernel_dense_and_csr(K, V, S, n, dtype):
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    ws = counts(n, V, seed=K + V, top=200)
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(dtype)
    fused_case(m, eng, ws, eps, S, what=f"K={K} V={V} S={S} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_fused_kernel_with_a_mean_function(dtype):
    K, n, S = 5, 70, 64
    m = build(K, n, dtype, mean_function=MEAN_KN)
    eng = engine(m, dtype)
    ws = counts(n, m.V, seed=3, top=200)
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    fused_case(m, eng, ws, eps, S, mean=dev(MEAN_KN(m.xs), eng), what=f"mean_function {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [9, 131])
def test_philox_draws_do_not_depend_on_how_the_rows_are_cut(V, dtype):
    """(e): one call against pieces of 1, RP and RP + 1 rows, each with its row_offset, bit for bit, dense and CSR; and against the eps
    path fed with the same draws"""
    K, n, S, seed, off = 5, 70, 64, 0x1234ABCD5678, 1000
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(counts(n, V, seed=2, top=200), eng, torch.int32)
    E = torch.stack([eng.fill_eps(seed, s, off, n) for s in range(S)]).contiguous()
    for name, w, rows in (("dense", ws, lambda a, b: ws[a:b].contiguous()), ("csr", to_csr(ws), lambda a, b: csr_rows(to_csr(ws), slice(a, b)))):
        one, a_one = eng.predict_loo(xs, w, S, seed=seed, row_offset=off, return_log_lik=True)
        RP = eng.last_loo_plan()["RP"]
        for size in (1, RP, RP + 1):
            parts = [eng.predict_loo(xs[a:a + size].contiguous(), rows(a, min(n, a + size)), S, seed=seed, row_offset=off + a, return_log_lik=True)
                     for a in range(0, n, size)]
            assert same(torch.cat([p[0] for p in parts], 1), one) and torch.equal(torch.cat([p[1] for p in parts], 1), a_one), (name, size)
        inj, a_inj = eng.predict_loo(xs, w, S, eps=E, return_log_lik=True)
        assert float((a_inj - a_one).abs().max()) / float(a_one.abs().max()) < TOL[dtype], name
        assert float((inj[ELPD] - one[ELPD]).abs().max()) / float(one[ELPD].abs().max()) < TOL[dtype], name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_surface(dtype, monkeypatch):
    """(g): pointwise_loo, loo and psis on the model, over row pieces, dense and CSR"""
    import gdrf_amd.models.sparse_gdrf as sg
    from gdrf_amd.models import compare_pointwise, loo_from_pointwise
    K, n, S = 5, 257, 64
    m = build(K, n, dtype, mean_function=MEAN_KN)
    xs, ws = m.xs.to(dtype), counts(n, m.V, seed=6, top=200)
    big = _model(m, dtype, n, mean_function=MEAN_KN)
    whole = big.pointwise_loo(xs, ws, S, seed=3, return_log_lik=True)
    assert tuple(whole) == LOO_NAMES + ("log_lik",) and whole["log_lik"].shape == (S, n)
    assert all(whole[k].shape == (n,) and whole[k].dtype == torch.float64 for k in LOO_NAMES)
    assert tuple(big.pointwise_loo(xs, ws, S, seed=3)) == LOO_NAMES
    # lpd, total and log_coef are pointwise_log_likelihood's
    pl = big.pointwise_log_likelihood(xs, ws, S, seed=3)
    assert all(torch.equal(whole[k], pl[k]) for k in ("lpd", "total", "log_coef"))
    # pieces of 64 rows change nothing, dense or CSR
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 64)
    small = _model(m, dtype, 64, mean_function=MEAN_KN)
    wc = to_csr(ws)
    cut, cut_csr, whole_csr = small.pointwise_loo(xs, ws, S, seed=3, return_log_lik=True), small.pointwise_loo(xs, wc, S, seed=3), \
        big.pointwise_loo(xs, wc, S, seed=3)
    assert small._engine.n_cap == 64
    for name in LOO_NAMES:
        assert same(whole[name], cut[name]) and same(whole_csr[name], cut_csr[name]), name
    assert torch.equal(whole["log_lik"], cut["log_lik"])
    # normalized=True shifts elpd_loo and lpd by log_coef and nothing else
    norm = big.pointwise_loo(xs, ws, S, seed=3, normalized=True)
    assert torch.equal(norm["elpd_loo"], whole["elpd_loo"] + whole["log_coef"]) and torch.equal(norm["lpd"], whole["lpd"] + whole["log_coef"])
    assert all(same(norm[k], whole[k]) for k in ("pareto_k", "ess", "total", "log_coef"))
    # the held-out density is never above the within-sample one (the weights fall as the likelihood rises), row by row: p_loo >= 0
    slack = 1e-12 * float(whole["lpd"].abs().max())
    assert bool((whole["elpd_loo"] <= whole["lpd"] + slack).all())
    assert bool(((whole["ess"] > 1.0 - 1e-9) & (whole["ess"] <= S * (1.0 + 1e-9))).all())
    # loo is loo_from_pointwise of the maps
    r = big.loo(xs, ws, S, seed=3)
    want = loo_from_pointwise(whole, S)
    assert torch.equal(r["pointwise"], whole["elpd_loo"]) and torch.equal(r["elpd_loo"], want["elpd_loo"]) and float(r["looic"]) == -2.0 * float(r["elpd_loo"])
    assert float(r["p_loo"]) >= -slack * n and float(r["se"]) > 0 and r["k_threshold"] == min(1.0 - 1.0 / math.log10(S), 0.7)
    assert r["n_not_fitted"] == int(torch.isnan(whole["pareto_k"]).sum()) >= 1 and r["n_bad_k"] == int((whole["pareto_k"] > r["k_threshold"]).sum())
    rn = big.loo(xs, ws, S, seed=3, normalized=True)
    assert abs(float(rn["elpd_loo"]) - float(r["elpd_loo"]) - float(whole["log_coef"].sum())) < 1e-9 * abs(float(rn["elpd_loo"]))
    assert abs(float(rn["p_loo"]) - float(r["p_loo"])) < 1e-9 * abs(float(r["elpd_loo"]))
    # LOO beside WAIC on the same rows, paired
    cmp = compare_pointwise(r["pointwise"], big.waic(xs, ws, S, seed=3)["pointwise"])
    assert math.isfinite(float(cmp["elpd_diff"])) and float(cmp["se_diff"]) >= 0
    # psis on the matrix the model returned: the fused maps, to the caps, in pieces of n_cap columns too
    for model in (big, small):
        st = model.psis(whole["log_lik"])
        assert tuple(st) == LOO_NAMES[:3]
        held(torch.stack([st[k] for k in LOO_NAMES[:3]]), torch.stack([whole[k] for k in LOO_NAMES[:3]]), whole["log_lik"], f"model.psis {dtype}")
    # a custom link is refused and pointed at psis
    linked = _model(m, dtype, 64, link_function=lambda mu: torch.softmax(mu, -2), mean_function=MEAN_KN)
    for call in (linked.pointwise_loo, linked.loo):
        with pytest.raises(NotImplementedError, match="psis"):
            call(xs, ws, S)
    assert linked.psis(whole["log_lik"].cpu())["elpd_loo"].shape == (n,)


def test_refusals():
    """(h)"""
    import ctypes as C
    from gdrf_amd import _lib
    m = build(5, 63, torch.float64)
    eng = engine(m, torch.float64, n_cap=32)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    x8, w8 = xs[:8].contiguous(), ws[:8].contiguous()
    for S in (24, 1025):
        with pytest.raises(ValueError, match="25 .. 1024"):
            eng.predict_loo(x8, w8, S, seed=1)
        with pytest.raises(ValueError, match="25 .. 1024"):
            eng.psis_rows(torch.zeros(S, 4, dtype=torch.float64, device=eng.device))
    with pytest.raises(ValueError, match="ws must be counts of shape"):
        eng.predict_loo(x8, ws[:9].contiguous(), 32, seed=1)
    with pytest.raises(ValueError, match="eps must have shape"):
        eng.predict_loo(x8, w8, 32, eps=torch.zeros(31, 5, 8, dtype=torch.float64, device=eng.device))
    with pytest.raises(ValueError, match="n_cap"):
        eng.predict_loo(xs, ws, 32, seed=1)
    with pytest.raises(ValueError, match="seed"):
        eng.predict_loo(x8, w8, 32)
    with pytest.raises(ValueError, match="float64"):
        eng.psis_rows(torch.zeros(32, 4, dtype=torch.float32, device=eng.device))
    # the library's own refusals, reached past the Python checks
    a = torch.zeros(32, 4, dtype=torch.float64, device=eng.device)
    out = torch.empty(3, 4, dtype=torch.float64, device=eng.device)
    for args, word in (((a.data_ptr(), 32, loo_tail_len(32) + 1, 4, out.data_ptr()), "tail_len"), ((a.data_ptr(), 24, 5, 4, out.data_ptr()), "num_samples"),
                       ((a.data_ptr(), 32, 7, 0, out.data_ptr()), "n must be"), ((a.data_ptr(), 32, 7, 4, None), "out is required")):
        with pytest.raises(_lib.GdrfHipError, match=word):
            _lib.check(eng.lib.gdrf_psis_rows(eng.ctx, *args, None), "gdrf_psis_rows")
    o6 = torch.empty(6, 8, dtype=torch.float64, device=eng.device)
    base = [eng.ctx, x8.data_ptr(), 8, eng.Z.data_ptr(), eng.params.data_ptr(), w8.data_ptr(), None, None, None, 32, 7, C.c_uint64(1), 0, None,
            o6.data_ptr(), None, None]
    for change, word in (({5: None}, "either dense"), ({6: w8.data_ptr()}, "either dense"), ({2: 33}, "n_cap"), ({10: 6}, "tail_len"), ({9: 1025, 10: 96}, "num_samples"),
                         ({14: None}, "out is required")):
        args = list(base)
        for i, v in change.items():
            args[i] = v
        with pytest.raises(_lib.GdrfHipError, match=word):
            _lib.check(eng.lib.gdrf_predict_loo(*args), "gdrf_predict_loo")
    assert eng.predict_loo(x8, w8, 25, seed=1).shape == (6, 8) and eng.predict_loo(x8, w8, 1024, seed=1).shape == (6, 8)
