"""GPU tests of the per-row Monte-Carlo log predictive densities and WAIC (gdrf_predict_score, csrc/predict_score.h) against the float64
restatement of tests/_score_ref.py, on the model of tests/test_gpu_predict_mc.py (grid model M = 20, variance 25, perturbed u_loc /
phi_unc, contracted u_scale_tril; float32 contexts at float32-valued parameters and the same jitter level) with counts whose row totals
run up to 1e4 (tests/_score_ref.py::counts).

Tolerances.  lpd and mean_log_lik (and row_perplexity): the predictive path's TOL, 1e-9 in fp64 contexts and 5e-4 in float32 ones, as
max-abs error over max-abs value.  total is exact; log_coef is formed in double in either context and held to 1e-9.  var_log_lik is a
variance of large, nearly equal sums; its error is taken relative to the case's largest var_log_lik, 1e-9 in fp64 contexts.  Its float32
error had not been measured before this file: VAR_TOL[float32] is four times the worst value seen on an MI355X over every injected-eps
case below (MEASURED has the figures per test: 2.29e-5 at worst, at V = 20000, and 3.8e-6 over the K x n x S sweep); that is room for
other draws, not for another algorithm.  A float32 context solves in float64, so its f_loc and f_var are good to about 1e-7; what is
left is the float32 log of p under counts of up to 1e4.
V = 1 (every a_s is 0) is held absolutely instead: tests/_score_ref.py::errors has the reasoning; the largest var_log_lik seen there is
0.002 of its bound.
"""
import copy
import math

import pytest
import torch

from gdrf_amd.data import csr_rows, to_csr
from gdrf_amd.engine import SCORE_NAMES, SCORE_S_TILE, SCORE_V_CHUNK
from tests._score_ref import COEF, LPD, MLL, NAMES, TOL, TOT, VLL, counts, errors, log_liks, score_ref, stats
from tests._util import dev, relerr
from tests._mc_util import MEAN_KN, _model, build, engine

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
KS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128)                 # both sides of every lane-group form
NS = (1, 63, 257)                                           # a partly filled last workgroup pass
T, C = SCORE_S_TILE, SCORE_V_CHUNK
SS = (1, 2, T - 1, T, T + 1, 2 * T + 2)                     # the tile edges
VS = (1, C - 1, C, C + 1, 2 * C + 3)                        # the chunk edges
# The worst float32 var_log_lik error (max-abs over the case's largest var_log_lik, against the float64 restatement) seen per test on an
# MI355X, row totals up to 1e4:
MEASURED = {"every_form_and_shape": 3.81e-6, "chunk_edges": 3.03e-6, "csr_rows": 9.79e-6, "large_vocabulary": 2.29e-5, "variants": 2.60e-6,
            "model": 3.09e-7}                               # in fp64 contexts the worst is 7.5e-14; lpd and mean_log_lik: 3.3e-7 and 6.4e-15
VAR_TOL = {torch.float64: 1e-9, torch.float32: 4 * 2.29e-5}          # four times the worst of the first measurement, 9.2e-5; it stays


def lane_group(K):
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def check(eng, m, xs, ws, eps, mean=None, sparse=False, ref=None):
    """all five outputs with injected eps against the restatement; ``ws`` dense on the host, handed over dense or as CSR"""
    S, K, n = eps.shape
    ref = score_ref(m, xs, ws, eps) if ref is None else ref
    wd = dev(ws, eng, torch.int32)
    out = eng.predict_score(dev(xs, eng), to_csr(wd) if sparse else wd, S, eps=dev(eps, eng), mean=mean)
    assert out.shape == (5, n) and out.dtype == torch.float64
    one_word = (K + 8) * torch.finfo(eng.dtype).eps if m.V == 1 else 0.0       # V = 1: the most |p - 1| can be (tests/_score_ref.py::errors)
    figs = errors(out, ref, one_word=one_word)
    print(f"K={K} V={m.V} n={n} S={S} {'csr' if sparse else 'dense'} {eng.dtype}", {k: f"{v:.2e}" for k, v in figs.items()})
    tol = TOL[eng.dtype]
    assert figs["lpd"] < tol and figs["mean_log_lik"] < tol, figs
    assert figs["var_log_lik"] <= (1.0 if one_word else VAR_TOL[eng.dtype]), figs
    assert figs["total"] == 0.0 and figs["log_coef"] < 1e-9, figs
    return out


def test_names_and_constants_match_the_reference_module():
    assert SCORE_NAMES == NAMES and (T, C) == (64, 128)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", KS)
def test_injected_eps_parity_every_form_and_shape(K, dtype):
    m = build(K, max(NS), dtype)
    eng = engine(m, dtype)
    ws = counts(max(NS), m.V, seed=K)
    g = torch.Generator().manual_seed(7)
    for n in NS:
        for S in SS:
            eps = torch.randn(S, K, n, generator=g, dtype=torch.float64).to(dtype)
            xs_n, ws_n = m.xs[:n].contiguous(), ws[:n].contiguous()
            ref = score_ref(m, xs_n, ws_n, eps)
            for sparse in (False, True):                    # the tiles are the dense form's; the CSR form takes every S as well
                check(eng, m, xs_n, ws_n, eps, sparse=sparse, ref=ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [5, 128])
@pytest.mark.parametrize("V", VS)
def test_injected_eps_parity_at_the_chunk_edges_dense_and_csr(V, K, dtype):
    """more than one chunk under more than one tile; K = 128, V = 129 in float64 is the largest launch (136 KB of LDS): it must fit"""
    n, S = 63, T + 1
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    ws = counts(n, V, seed=V)
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    ref = score_ref(m, m.xs, ws, eps)
    dense = check(eng, m, m.xs, ws, eps, ref=ref)
    sparse = check(eng, m, m.xs, ws, eps, ref=ref, sparse=True)
    assert torch.equal(dense[TOT], sparse[TOT])
    assert relerr(sparse[COEF].cpu().numpy(), dense[COEF].cpu().numpy()) < 1e-9
    for i in (LPD, MLL):                                    # the two forms add a row's words in different orders
        assert relerr(sparse[i].cpu().numpy(), dense[i].cpu().numpy()) < TOL[dtype], NAMES[i]


def csr_edge_counts(LG, V, seed):
    """(CSR on the host, the same counts dense): rows with 0, LG - 1, LG, LG + 1 and 2 LG + 3 stored entries, stored zeros among them, a
    row whose only entry is a stored zero, and a last row without entries"""
    g = torch.Generator().manual_seed(seed)
    nnz = [0, LG - 1, LG, LG + 1, 2 * LG + 3, 1, 0]
    crow, cols, vals = [0], [], []
    dense = torch.zeros(len(nnz), V, dtype=torch.int32)
    for r, c in enumerate(nnz):
        cc = torch.randperm(V, generator=g)[:c].sort().values
        vv = torch.randint(1, 2000, (c,), generator=g, dtype=torch.int32)
        if c >= 3:
            vv[1] = vv[c - 1] = 0
        if c == 1:
            vv[0] = 0
        dense[r, cc] = vv
        cols.append(cc)
        vals.append(vv)
        crow.append(crow[-1] + c)
    ws = torch.sparse_csr_tensor(torch.tensor(crow, dtype=torch.int64), torch.cat(cols).to(torch.int64), torch.cat(vals), size=(len(nnz), V))
    return ws, dense


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [5, 9, 17, 65])
def test_csr_rows_with_every_entry_count_round_the_group_width(K, dtype):
    LG = lane_group(K)
    V, S = 2 * LG + 12, 7
    ws, dense = csr_edge_counts(LG, V, seed=K)
    n = dense.shape[0]
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    ref = score_ref(m, m.xs, dense, eps)
    xs, ed = dev(m.xs, eng), dev(eps, eng)
    out = eng.predict_score(xs, ws.to(eng.device), S, eps=ed)
    figs = errors(out, ref)
    print(f"K={K} LG={LG} V={V} {dtype}", {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["lpd"] < TOL[dtype] and figs["mean_log_lik"] < TOL[dtype] and figs["var_log_lik"] < VAR_TOL[dtype], figs
    assert figs["total"] == 0.0 and figs["log_coef"] < 1e-9, figs
    for r in (0, 5, 6):                                     # no entry, a stored zero alone, no entry: five zeros
        assert torch.equal(out[:, r], torch.zeros(5, dtype=torch.float64, device=out.device)), r
    # the stored zeros are absent entries: the matrix without them (its entries fall to other lanes) and the dense form agree to rounding
    again = eng.predict_score(xs, to_csr(dev(dense, eng, torch.int32)), S, eps=ed)
    assert torch.equal(out[TOT], again[TOT])
    assert all(relerr(again[i].cpu().numpy(), out[i].cpu().numpy()) < (1e-9 if i == COEF else TOL[dtype]) for i in (LPD, MLL, COEF))
    full = eng.predict_score(xs, dev(dense, eng, torch.int32), S, eps=ed)
    assert torch.equal(full[TOT], out[TOT]) and relerr(full[COEF].cpu().numpy(), out[COEF].cpu().numpy()) < 1e-9
    assert relerr(full[LPD].cpu().numpy(), out[LPD].cpu().numpy()) < TOL[dtype] and relerr(full[MLL].cpu().numpy(), out[MLL].cpu().numpy()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_an_all_empty_matrix_scores_zero_everywhere(sparse, dtype):
    K, n, S = 5, 63, 3
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    ws = torch.zeros(n, m.V, dtype=torch.int32, device=eng.device)
    out = eng.predict_score(dev(m.xs, eng), to_csr(ws) if sparse else ws, S, seed=3)
    assert torch.equal(out, torch.zeros(5, n, dtype=torch.float64, device=eng.device))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_large_sparse_vocabulary_is_scored_where_the_summed_score_refuses(dtype):
    from gdrf_amd._lib import GdrfHipError
    K, n, S, V = 5, 63, 7, 20000
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    g = torch.Generator().manual_seed(5)
    ws = torch.zeros(n, V, dtype=torch.int32)
    for r in range(n):                                      # at most 40 stored entries a row, row 0 has none
        c = torch.randperm(V, generator=g)[:(r * 7) % 41]
        ws[r, c] = torch.randint(1, 500, (c.numel(),), generator=g, dtype=torch.int32)
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    ref = score_ref(m, m.xs, ws, eps)
    sparse = check(eng, m, m.xs, ws, eps, ref=ref, sparse=True)
    dense = check(eng, m, m.xs, ws, eps, ref=ref)          # 157 chunks
    assert relerr(sparse[LPD].cpu().numpy(), dense[LPD].cpu().numpy()) < TOL[dtype]
    # the summed score keeps its limits: Phi does not fit its LDS, and it reads no CSR
    xs, wd = dev(m.xs, eng), dev(ws, eng, torch.int32)
    with pytest.raises(GdrfHipError, match="too large"):
        eng.predict_mc(xs, 2, S, ws=wd, seed=1)
    with pytest.raises(ValueError, match="dense counts"):
        eng.predict_mc(xs, 2, S, ws=to_csr(wd), seed=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["mean_function", "unwhitened", "matern52"])
def test_injected_eps_parity_mean_unwhitened_and_matern(variant, dtype):
    mean_fn = MEAN_KN if variant == "mean_function" else None
    m = build(5, 63, dtype, kind="matern52" if variant == "matern52" else "rbf", whiten=variant != "unwhitened", mean_function=mean_fn)
    eng = engine(m, dtype)
    eps = torch.randn(7, 5, 63, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    mean = None if mean_fn is None else dev(mean_fn(m.xs), eng)
    ws = counts(63, m.V, seed=3)
    check(eng, m, m.xs, ws, eps, mean=mean)
    check(eng, m, m.xs, ws, eps, mean=mean, sparse=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [9, 2 * C + 3])
def test_zero_eps_is_the_plug_in_with_no_variance(V, dtype):
    K, n, S = 5, 257, 3
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(counts(n, V, seed=4), eng, torch.int32)
    zero = torch.zeros(S, K, n, dtype=dtype, device=eng.device)
    plug = eng.predict(xs, 3, ws).cpu().numpy()              # {sum w log p, sum w} at softmax(f_loc)
    for w in (ws, to_csr(ws)):
        out = eng.predict_score(xs, w, S, eps=zero)
        assert torch.equal(out[LPD], out[MLL]) and torch.equal(out[VLL], torch.zeros_like(out[VLL]))
        assert abs(float(out[LPD].sum()) - plug[0]) / abs(plug[0]) < TOL[dtype] and float(out[TOT].sum()) == plug[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_topic_does_not_see_the_draws(dtype):
    n, S = 63, T + 3
    m = build(1, n, dtype)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(counts(n, m.V, seed=4), eng, torch.int32)
    for w in (ws, to_csr(ws)):
        one = eng.predict_score(xs, w, 1, seed=9)
        out = eng.predict_score(xs, w, S, seed=3)
        assert torch.equal(out[VLL], torch.zeros_like(out[VLL])) and torch.equal(out[MLL], one[MLL])
        assert relerr(out[LPD].cpu().numpy(), one[LPD].cpu().numpy()) < 1e-14          # log(S x 1) - log S, rounded once
    assert float(one[LPD].abs().max()) > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,S", [(5, 64), (33, 7)])
def test_the_rows_sum_to_the_summed_score_at_the_same_seed(K, S, dtype):
    n, seed = 257, 20240229
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws[:n], eng, torch.int32)
    out = eng.predict_score(xs, ws, S, seed=seed)
    summed = eng.predict_mc(xs, 2, S, ws=ws, seed=seed).cpu().numpy()
    assert float(out[TOT].sum()) == summed[1]
    a, b = math.exp(-float(out[LPD].sum()) / float(out[TOT].sum())), math.exp(-summed[0] / summed[1])
    print(dtype, "perplexity from the rows", a, "from the summed score", b)
    assert abs(a - b) / b < TOL[dtype]
    # Jensen: the log of the mean is at least the mean of the logs, and the variance is not negative
    assert bool((out[LPD] >= out[MLL] - TOL[dtype] * out[MLL].abs().max()).all()) and bool((out[VLL] >= 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,n,S,off,V", [(5, 63, 7, 1000, 9), (128, 257, 2, 2 ** 33 + 5, 9), (2, 1, T + 1, 0, 9), (9, 63, 3, 7, C + 3)])
def test_philox_draws_equal_their_own_injection_bitwise(K, n, S, off, V, dtype):
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(counts(n, V, seed=2), eng, torch.int32)
    seed = 0x1234ABCD5678
    E = torch.stack([eng.fill_eps(seed, s, off, n) for s in range(S)]).contiguous()
    for w in (ws, to_csr(ws)):
        assert torch.equal(eng.predict_score(xs, w, S, seed=seed, row_offset=off), eng.predict_score(xs, w, S, eps=E))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [9, C + 3])
def test_results_do_not_depend_on_how_the_rows_are_batched(V, dtype):
    K, n, S = 5, 257, T + 1
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(counts(n, V, seed=2), eng, torch.int32)
    eps = dev(torch.randn(S, K, n, generator=torch.Generator().manual_seed(3), dtype=torch.float64), eng)
    cuts = (0, 1, 101, 257)
    for name, w, rows in (("dense", ws, lambda a, b: ws[a:b].contiguous()), ("csr", to_csr(ws), lambda a, b: csr_rows(to_csr(ws), slice(a, b)))):
        one = eng.predict_score(xs, w, S, seed=11)
        assert torch.equal(one, eng.predict_score(xs, w, S, seed=11)), name
        pieces = torch.cat([eng.predict_score(xs[a:b].contiguous(), rows(a, b), S, seed=11, row_offset=a) for a, b in zip(cuts[:-1], cuts[1:])], dim=1)
        assert torch.equal(one, pieces), name
        one = eng.predict_score(xs, w, S, eps=eps)
        assert torch.equal(one, eng.predict_score(xs, w, S, eps=eps)), name
        pieces = torch.cat([eng.predict_score(xs[a:b].contiguous(), rows(a, b), S, eps=eps[:, :, a:b].contiguous()) for a, b in zip(cuts[:-1], cuts[1:])], dim=1)
        assert torch.equal(one, pieces), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_surface_cuts_rows_into_pieces_without_changing_the_result(dtype, monkeypatch):
    import gdrf_amd.models.sparse_gdrf as sg
    from gdrf_amd.models import waic_from_pointwise
    K, n, S = 5, 257, 7
    m = build(K, n, dtype, mean_function=MEAN_KN)
    xs, ws = m.xs.to(dtype), counts(n, m.V, seed=6)
    big = _model(m, dtype, n, mean_function=MEAN_KN)
    whole = big.pointwise_log_likelihood(xs, ws, S, seed=3)
    assert big._engine.n_cap == n and tuple(whole) == NAMES
    assert all(v.shape == (n,) and v.dtype == torch.float64 for v in whole.values())
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 64)
    small = _model(m, dtype, 64, mean_function=MEAN_KN)
    wc = to_csr(ws)
    cut, cut_csr, whole_csr = small.pointwise_log_likelihood(xs, ws, S, seed=3), small.pointwise_log_likelihood(xs, wc, S, seed=3), \
        big.pointwise_log_likelihood(xs, wc, S, seed=3)
    assert small._engine.n_cap == 64
    for name in NAMES:
        assert torch.equal(whole[name], cut[name]) and torch.equal(whole_csr[name], cut_csr[name]), name
    # seed=None is the model's rng_seed; normalized=True shifts lpd and mean_log_lik by log_coef and nothing else
    assert torch.equal(small.pointwise_log_likelihood(xs, ws, 2)["lpd"], small.pointwise_log_likelihood(xs, ws, 2, seed=small.rng_seed)["lpd"])
    norm = big.pointwise_log_likelihood(xs, ws, S, seed=3, normalized=True)
    assert torch.equal(norm["lpd"], whole["lpd"] + whole["log_coef"]) and torch.equal(norm["mean_log_lik"], whole["mean_log_lik"] + whole["log_coef"])
    for name in ("var_log_lik", "total", "log_coef"):
        assert torch.equal(norm[name], whole[name]), name
    # against the restatement, with the mean_function, through injected draws cut into the same pieces
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype)
    m.force_jitter_level = small._engine.last_jitter_level
    a = log_liks(m, m.xs, ws, eps)
    ref = stats(a, ws)
    got = small.pointwise_log_likelihood(xs, wc, S, eps=eps)
    figs = errors(torch.stack([got[k] for k in NAMES]), ref)
    print(dtype, {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["lpd"] < TOL[dtype] and figs["mean_log_lik"] < TOL[dtype] and figs["var_log_lik"] < VAR_TOL[dtype], figs
    assert figs["total"] == 0.0 and figs["log_coef"] < 1e-9, figs
    # WAIC is waic_from_pointwise of the maps; the surprise map is exp(-lpd / total), NaN on the empty last row
    w = big.waic(xs, ws, S, seed=3)
    want = waic_from_pointwise(whole)
    assert torch.equal(w["pointwise"], whole["lpd"] - whole["var_log_lik"]) and torch.equal(w["elpd_waic"], want["elpd_waic"])
    assert float(w["waic"]) == -2.0 * float(w["elpd_waic"]) and float(w["p_waic"]) == float(whole["var_log_lik"].sum())
    assert w["n_high_variance"] == int((whole["var_log_lik"] > 0.4).sum()) and float(w["se"]) > 0
    wn = big.waic(xs, ws, S, seed=3, normalized=True)
    assert abs(float(wn["elpd_waic"]) - float(w["elpd_waic"]) - float(whole["log_coef"].sum())) < 1e-9 * abs(float(wn["elpd_waic"]))
    rp = big.row_perplexity(xs, ws, S, seed=3)
    assert rp.shape == (n,) and rp.dtype == torch.float64 and bool(torch.isnan(rp[-1])) and not bool(torch.isnan(rp[:-1]).any())
    assert torch.equal(rp[:-1], torch.exp(-whole["lpd"][:-1] / whole["total"][:-1]))
    ref_rp = torch.exp(-ref[LPD][:-1] / ref[TOT][:-1])
    got_rp = torch.exp(-got["lpd"][:-1] / got["total"][:-1]).cpu()
    assert relerr(got_rp.numpy(), ref_rp.numpy()) < TOL[dtype]
    # the rows and the summed score tell the same perplexity; the summed score still refuses CSR counts
    pa = math.exp(-float(whole["lpd"].sum()) / float(whole["total"].sum()))
    assert abs(pa - float(big.predictive_perplexity(xs, ws, S, seed=3))) / pa < TOL[dtype]
    with pytest.raises(ValueError, match="dense counts"):
        big.predictive_perplexity(xs, wc, S, seed=3)
    # a restored snapshot offers the same methods; a custom link is refused
    snap = copy.deepcopy(big)
    again = snap.restore(mean_function=MEAN_KN).pointwise_log_likelihood(xs, ws, S, seed=3)
    assert relerr(again["lpd"].cpu().numpy(), whole["lpd"].cpu().numpy()) < TOL[dtype]
    linked = _model(m, dtype, 64, link_function=lambda mu: torch.softmax(mu, -2), mean_function=MEAN_KN)
    for call in (linked.pointwise_log_likelihood, linked.waic, linked.row_perplexity):
        with pytest.raises(NotImplementedError):
            call(xs, ws, S)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_step_is_bitwise_the_same_after_predict_score(dtype):
    K, n = 5, 63
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    eps = dev(torch.randn(K, n, generator=torch.Generator().manual_seed(4), dtype=torch.float64), eng)

    def step():
        eng.loss_and_grads(xs, ws, eps)
        return eng.out_d.clone(), eng.grads.clone()

    step()
    out1, g1 = step()
    for w in (ws[:40].contiguous(), to_csr(ws[:40].contiguous())):
        eng.predict_score(xs[:40].contiguous(), w, 3, seed=1, mean=dev(torch.ones(40), eng))
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)


def test_limits():
    m = build(5, 63, torch.float64)
    eng = engine(m, torch.float64, n_cap=32)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    with pytest.raises(ValueError, match="n_cap"):
        eng.predict_score(xs, ws, 2, seed=1)
    with pytest.raises(ValueError, match="seed"):
        eng.predict_score(xs[:8].contiguous(), ws[:8].contiguous(), 2)
    with pytest.raises(ValueError, match="int32"):
        eng.predict_score(xs[:8].contiguous(), ws[:8].long().contiguous(), 2, seed=1)
    assert eng.predict_score(xs[:8].contiguous(), ws[:8].contiguous(), 65535, seed=1).shape == (5, 8)
