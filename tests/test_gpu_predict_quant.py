"""GPU tests of the credible-interval, exceedance and dominant-topic maps (gdrf_predict_quant, csrc/predict_quant.h) on the model of
tests/test_gpu_predict_mc.py (grid model M = 20, variance 25, perturbed u_loc / phi_unc, contracted u_scale_tril).

Topics: the kernel's samples are the bits of predict_mc's mode 0 under the same arguments, so against tests/_quant_ref.py applied to
those samples the extreme quantiles, the exceedance counts and the dominance counts are exact and an interpolated quantile is within
8 * 2^-53 * max(|x_lo|, |x_hi|) - three double roundings in the restatement and at most three on the device, fused or not, each bounded
by the larger endpoint.  Words: against theta (double) times softmax(phi_unc) (double), band b = (K + 8) eps(T) relative - K products
and sums of positive terms in T, a few eps for Phi's exp, sum and divide in T.
"""
import copy
import math
from statistics import NormalDist

import pytest
import torch

from gdrf_amd.engine import QUANT_DOMINANT, QUANT_EXCEED, QUANT_QUANTILE
from tests import _quant_ref as QR
from tests._info_ref import TOL
from tests._util import dev, relerr
from tests._mc_util import MEAN_KN, _model, build, engine

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
KS = (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128)              # both sides of every lane-group form
NS, SS = (1, 63, 257), (1, 2, 3, 7, 64, 65)
QS = (0.0, 0.025, 1.0 / 3.0, 0.5, 0.9, 1.0)
ULP = 2.0 ** -53
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}


def taus_for(K):
    return (-1.0, 0.0, 1.0 / K, 0.5, 1.0, 2.0)


def check_topics(eng, xs_d, S, **kw):
    """the three modes over topics against the restatement applied to the engine's own samples under the same arguments"""
    K, n = eng.K, xs_d.shape[0]
    th = eng.predict_mc(xs_d, 0, S, **kw).cpu()
    out = eng.predict_quant(xs_d, QUANT_QUANTILE, S, levels=QS, **kw).cpu()
    assert out.shape == (len(QS), n, K) and out.dtype == torch.float64
    assert torch.equal(out[0], th.min(0).values.double()) and torch.equal(out[-1], th.max(0).values.double())
    ref, ends = QR.quantiles_ref(th, QS), QR.quantile_ends(th, QS)
    worst = float(((out - ref).abs() / ends.clamp_min(1e-300)).max()) / ULP
    assert bool(((out - ref).abs() <= 8 * ULP * ends).all()), f"K={K} n={n} S={S}: {worst:.2f} ulp"
    taus = taus_for(K)
    ex = eng.predict_quant(xs_d, QUANT_EXCEED, S, levels=taus, **kw).cpu()
    assert ex.shape == (len(taus), n, K) and ex.dtype == torch.float64
    assert torch.equal(ex, QR.exceed_ref(th, taus))
    assert bool((ex[0] == 1).all()) and bool((ex[4] == 0).all()) and bool((ex[5] == 0).all())
    dm = eng.predict_quant(xs_d, QUANT_DOMINANT, S, **kw).cpu()
    assert dm.shape == (n, K) and dm.dtype == torch.float64
    assert torch.equal(dm, QR.dominant_ref(th))
    cnt = (dm * S).round()
    assert bool(((dm * S - cnt).abs() < 1e-9).all()) and bool((cnt.sum(-1) == S).all())
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", KS)
def test_topics_are_exact_against_the_engines_own_samples(K, dtype):
    m = build(K, max(NS), dtype)
    eng = engine(m, dtype)
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for n in NS:
        xs_d = dev(m.xs[:n].contiguous(), eng)
        for S in SS:
            eps = dev(torch.randn(S, K, n, generator=g, dtype=torch.float64).to(dtype), eng)
            worst = max(worst, check_topics(eng, xs_d, S, eps=eps), check_topics(eng, xs_d, S, seed=11 + S, row_offset=5))
    print(f"K={K} {dtype}: interpolated quantiles within {worst:.2f} ulp of the larger endpoint")


@pytest.mark.parametrize("K,dtype", [(8, torch.float64), (128, torch.float32), (128, torch.float64)], ids=["K8-fp64", "K128-fp32", "K128-fp64"])
def test_the_two_ends_of_the_plan_at_1024_samples(K, dtype):
    n, S = 63, 1024
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    worst = check_topics(eng, dev(m.xs, eng), S, seed=3)
    eng.predict_quant(dev(m.xs, eng), QUANT_QUANTILE, S, levels=QS, seed=3)        # check_topics ends on a counter mode
    plan = eng.last_quant_plan()
    print(f"K={K} {dtype}: plan {plan}, {worst:.2f} ulp")
    assert (plan["RP"], plan["CP"], plan["lds"]) == QR.GPU_PLANS[(K, S, 8 if dtype == torch.float64 else 4)]


# ---- words
def word_samples(m, eng, xs_d, S, **kw):
    """p_s = theta_s (double) softmax(phi_unc) (double), (S, n, V), from the engine's own theta samples"""
    th = eng.predict_mc(xs_d, 0, S, **kw).cpu().double()
    with torch.no_grad():
        return th @ torch.softmax(m.params["phi_unc"].double(), -1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,V", [(5, 1), (5, 20), (5, 129), (8, 300), (128, 33)])
def test_words_against_theta_times_phi_in_double(K, V, dtype):
    n = 63
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs_d = dev(m.xs, eng)
    b = (K + 8) * EPS[dtype]
    g = torch.Generator().manual_seed(V)
    sub = torch.randperm(V, generator=g)[:max(1, min(V, 11))]
    lists = dict(all=None, subset=torch.cat([sub, sub[:1]]), single=torch.tensor([V // 2]))       # the subset ends on its first index again
    for S in (7, 64):
        p_all = word_samples(m, eng, xs_d, S, seed=21)
        for name, words in lists.items():
            idx = torch.arange(V) if words is None else words
            wd = dev(idx, eng, torch.int32)
            p = p_all[:, :, idx]
            out = eng.predict_quant(xs_d, QUANT_QUANTILE, S, levels=QS, words=wd, seed=21).cpu()
            assert out.shape == (len(QS), n, len(idx)) and out.dtype == torch.float64
            ref = QR.quantiles_ref(p, QS)
            rel = float(((out - ref).abs() / ref.abs()).max())
            print(f"K={K} V={V} S={S} {name} {dtype}: largest relative difference of p {rel:.2e} (b = {b:.2e})")
            assert bool(((out - ref).abs() <= b * p.abs().max(0).values).all()), rel
            assert bool((out[1:] >= out[:-1]).all())
            taus = (0.0, 0.5 / V, 1.5 / V, 3.0 / V, 2.0)            # none at p = 1, where the one-word model sits
            ex = eng.predict_quant(xs_d, QUANT_EXCEED, S, levels=taus, words=wd, seed=21).cpu()
            assert ex.shape == (len(taus), n, len(idx))
            cnt = (ex * S).round()
            assert bool(((ex * S - cnt).abs() < 1e-9).all())
            for t, tau in enumerate(taus):
                near = ((p - tau).abs() <= b * abs(tau)).sum(0)                  # samples whose side of tau the band does not decide
                assert int(near.sum()) <= 0.01 * p.numel(), (tau, int(near.sum()))
                assert bool(((cnt[t] - QR.exceed_counts_ref(p, (tau,))[0]).abs() <= near).all()), (name, tau)
            if name == "subset":
                assert torch.equal(out[:, :, 0], out[:, :, -1]) and torch.equal(ex[:, :, 0], ex[:, :, -1])
    with pytest.raises(ValueError, match="word"):
        eng.predict_quant(xs_d, QUANT_EXCEED, 7, levels=(0.5,), words=dev(torch.tensor([V]), eng, torch.int32), seed=1)


# ---- closed form at K = 2: theta_0 = sigmoid(mu_0 - mu_1), mu_0 - mu_1 ~ N(d, sg^2)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_topics_follow_the_logit_normal_closed_form(dtype):
    K, n, S, seed = 2, 257, 1024, 20240229
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs_d = dev(m.xs, eng)
    lv = eng.predict(xs_d, 4).cpu().double()
    d, sg = lv[0, 0] - lv[0, 1], (lv[1, 0] ** 2 + lv[1, 1] ** 2).sqrt()
    N01 = NormalDist()
    qs = (0.1, 0.5, 0.9)
    out = eng.predict_quant(xs_d, QUANT_QUANTILE, S, levels=qs, seed=seed).cpu()
    for i, q in enumerate(qs):
        # theta_1 = 1 - theta_0 up to rounding, so 1 - Q_q(theta_0) is Q_{1 - q}(theta_1): the logit without the cancellation near 1
        logit = out[i, :, 0].log() - out[len(qs) - 1 - i, :, 1].log()
        z = N01.inv_cdf(q)
        bound = 5 * sg * math.sqrt(q * (1 - q) / S) / N01.pdf(z) + TOL[dtype]
        err = (logit - (d + z * sg)).abs()
        print(f"{dtype} q={q}: largest error over bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
    taus = (0.25, 0.5, 0.75)
    ex = eng.predict_quant(xs_d, QUANT_EXCEED, S, levels=taus, seed=seed).cpu()
    for i, tau in enumerate(taus):
        p = 0.5 * (1 + torch.erf((d - math.log(tau / (1 - tau))) / sg / math.sqrt(2.0)))
        bound = 5 * (p * (1 - p) / S).sqrt() + 1.0 / S
        err = (ex[i, :, 0] - p).abs()
        print(f"{dtype} tau={tau}: largest error over bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


# ---- degenerate and invariant cases
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_eps_is_the_plug_in(dtype):
    K, n, S = 5, 257, 3
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs_d = dev(m.xs, eng)
    eps = torch.zeros(S, K, n, dtype=dtype, device=eng.device)
    out = eng.predict_quant(xs_d, QUANT_QUANTILE, S, levels=QS, eps=eps).cpu()
    want = eng.predict(xs_d, 1).cpu().double()
    for i in range(len(QS)):
        assert relerr(out[i].numpy(), want.numpy()) < TOL[dtype]
    ex = eng.predict_quant(xs_d, QUANT_EXCEED, S, levels=taus_for(K), eps=eps).cpu()
    assert bool(((ex == 0) | (ex == 1)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_topic_is_certain(dtype):
    m = build(1, 63, dtype)
    eng = engine(m, dtype)
    xs_d = dev(m.xs, eng)
    one = torch.ones(63, 1, dtype=torch.float64)
    out = eng.predict_quant(xs_d, QUANT_QUANTILE, 7, levels=QS, seed=3).cpu()
    assert torch.equal(out, one.expand(len(QS), 63, 1))
    assert torch.equal(eng.predict_quant(xs_d, QUANT_DOMINANT, 7, seed=3).cpu(), one)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,S", [(5, 64), (17, 7), (128, 65)])
def test_monotone_in_the_level_and_in_the_threshold(K, S, dtype):
    n = 257
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs_d = dev(m.xs, eng)
    qs = tuple(i / 15 for i in range(16))
    out = eng.predict_quant(xs_d, QUANT_QUANTILE, S, levels=qs, seed=5).cpu()
    assert bool((out[1:] >= out[:-1]).all()) and bool((out >= 0).all()) and bool((out <= 1).all())
    taus = tuple(sorted(torch.rand(16, generator=torch.Generator().manual_seed(1), dtype=torch.float64).tolist()))
    ex = eng.predict_quant(xs_d, QUANT_EXCEED, S, levels=taus, seed=5).cpu()
    assert bool((ex[1:] <= ex[:-1]).all()) and bool((ex >= 0).all()) and bool((ex <= 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["mean_function", "unwhitened", "matern52"])
def test_mean_unwhitened_and_matern_variants(variant, dtype):
    mean_fn = MEAN_KN if variant == "mean_function" else None
    m = build(5, 63, dtype, kind="matern52" if variant == "matern52" else "rbf", whiten=variant != "unwhitened", mean_function=mean_fn)
    eng = engine(m, dtype)
    mean = None if mean_fn is None else dev(mean_fn(m.xs), eng)
    eps = dev(torch.randn(7, 5, 63, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype), eng)
    check_topics(eng, dev(m.xs, eng), 7, eps=eps, mean=mean)
    check_topics(eng, dev(m.xs, eng), 7, seed=8, mean=mean)
    if mean is not None:                    # the mean is honoured: without it the median moves
        a = eng.predict_quant(dev(m.xs, eng), QUANT_QUANTILE, 7, levels=(0.5,), seed=8, mean=mean)
        assert not torch.equal(a, eng.predict_quant(dev(m.xs, eng), QUANT_QUANTILE, 7, levels=(0.5,), seed=8))


# ---- batching
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_results_do_not_depend_on_how_the_rows_are_batched(dtype):
    K, n, S, V = 5, 257, 65, 9
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs = dev(m.xs, eng)
    words = dev(torch.tensor([3, 0, 8, 3]), eng, torch.int32)
    calls = [(QUANT_QUANTILE, dict(levels=QS), 1), (QUANT_QUANTILE, dict(levels=QS, words=words), 1), (QUANT_EXCEED, dict(levels=taus_for(K)), 1),
             (QUANT_EXCEED, dict(levels=(0.1, 0.2), words=words), 1), (QUANT_DOMINANT, {}, 0)]
    for mode, kw, rows in calls:
        one = eng.predict_quant(xs, mode, S, seed=11, **kw)
        cut = torch.cat([eng.predict_quant(xs[a:b].contiguous(), mode, S, seed=11, row_offset=a, **kw) for a, b in ((0, 100), (100, 257))], dim=rows)
        assert torch.equal(one, cut), (mode, kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_surface_cuts_rows_into_pieces_without_changing_the_result(dtype, monkeypatch):
    import gdrf_amd.models.sparse_gdrf as sg
    K, n, S = 5, 257, 7
    m = build(K, n, dtype, mean_function=MEAN_KN)
    xs = m.xs.to(dtype)
    big = _model(m, dtype, n, mean_function=MEAN_KN)
    words = [3, 0, 8, 3]

    def surface(model):
        return dict(tq=model.topic_probs_quantiles(xs, QS, S, seed=3), wq=model.word_probs_quantiles(xs, QS, words, S, seed=3),
                    wq_all=model.word_probs_quantiles(xs, 0.5, None, S, seed=3), ex=model.exceedance(xs, 0.25, num_samples=S, seed=3),
                    exw=model.exceedance(xs, (0.05, 0.2), "word", words, S, seed=3), dom=model.dominant_topic_probs(xs, S, seed=3))

    whole = surface(big)
    assert big._engine.n_cap == n
    shapes = dict(tq=(len(QS), n, K), wq=(len(QS), n, 4), wq_all=(1, n, m.V), ex=(1, n, K), exw=(2, n, 4), dom=(n, K))
    for name, v in whole.items():
        assert v.shape == shapes[name] and v.dtype == torch.float64 and v.device.type == "cuda", name
    # the model's methods are the engine call on the prepared rows, with the mean_function's values
    xs_s, _ = big._prepare_inputs(xs)
    mean = big._mean_kn(big._mean_values(xs_s), n)
    assert torch.equal(whole["tq"], big._engine.predict_quant(xs_s, QUANT_QUANTILE, S, levels=QS, seed=3, mean=mean))
    assert torch.equal(whole["dom"], big._engine.predict_quant(xs_s, QUANT_DOMINANT, S, seed=3, mean=mean))
    assert not torch.equal(whole["tq"], big._engine.predict_quant(xs_s, QUANT_QUANTILE, S, levels=QS, seed=3))
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 64)
    small = _model(m, dtype, 64, mean_function=MEAN_KN)
    cut = surface(small)
    assert small._engine.n_cap == 64
    for name in whole:
        assert torch.equal(whole[name], cut[name]), name
    # seed=None is the model's rng_seed; an injected eps is cut with the rows
    assert torch.equal(small.dominant_topic_probs(xs, S), small.dominant_topic_probs(xs, S, seed=small.rng_seed))
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype)
    assert torch.equal(small.topic_probs_quantiles(xs, QS, S, eps=eps), big.topic_probs_quantiles(xs, QS, S, eps=eps))
    # a snapshot offers the same methods and gives the same bits
    again = surface(copy.deepcopy(big).restore(mean_function=MEAN_KN))
    for name in whole:
        assert torch.equal(whole[name], again[name]), name
    linked = _model(m, dtype, 64, link_function=lambda mu: torch.softmax(mu, -2), mean_function=MEAN_KN)
    with pytest.raises(NotImplementedError):
        linked.topic_probs_quantiles(xs, QS, S)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_step_is_bitwise_the_same_after_predict_quant(dtype):
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
    eng.predict_quant(xs[:40].contiguous(), QUANT_QUANTILE, 3, levels=QS, seed=1, mean=dev(torch.ones(40), eng))
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)
