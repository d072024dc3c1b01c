"""GPU tests of the posterior-predictive count sampler (gdrf_sample_counts, csrc/sample_counts.h) against a float64 torch restatement
of its definition, written here:

    p[s,n,v] = sum_k theta[s,n,k] Phi[k,v];  c[s,n,v] = p[s,n,0] + ... + p[s,n,v]
    word(s,n,t) = the smallest v with u[s,n,t] c[s,n,V-1] < c[s,n,v],  t < T_n;   w_rep[s,n,v] = #{ t : word(s,n,t) = v }
    deviance(w; q) = 2 sum_n sum_{v: w > 0} w log(w / (T_n q_v)),  q = p / c[V-1]

Counts carry no per-token record, so they are compared through a two-sided bound: a token is AMBIGUOUS when u c[V-1] lies within
m c[V-1] of an interior CDF value (m = 1e-12 in float64 contexts; 1e-4 in float32 ones, above the float32 error of p at K = 128, about
1e-5), its candidates are the words whose intervals meet that margin; every count lies between the unambiguous tokens of its word and
that plus the ambiguous tokens that have the word among their candidates, and every row sums to its total exactly.  The ambiguous share
of a call's tokens is asserted to be at most 10 % (uniform u give about 2 m (V - 1): 5.1 % at V = 257 in float32, nil in float64,
where the bound is an exact comparison).  The sums of mode 1 take the predictive path's tolerances (tests/test_gpu_predict_mc.py): 1e-9
in float64 contexts, 5e-4 in float32 ones, relerr of tests/_util.py.  The model is the recipe of tests/test_gpu_predict_mc.py.
"""
import copy
import math

import pytest
import torch

from tests._util import dev, relerr
from tests._mc_util import MEAN_KN, _model, build, engine

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-9, torch.float32: 5e-4}
MARGIN = {torch.float64: 1e-12, torch.float32: 1e-4}
DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
# V = 256 is the last size at which a wave owns a (row, sample) pair, 257 the first at which the workgroup does; Phi sits in LDS at the
# small K x V only
KS, VS, NS, SS = (1, 2, 5, 65, 128), (1, 2, 9, 63, 64, 65, 256, 257), (1, 63, 257), (1, 2, 7)
TOTALS = (0, 1, 3, 64, 65, 1000)
_ENGINES = {}


def eng_for(K, V, dtype, keep=True):
    """an engine and its oracle model; the few shapes several tests use are built once for the module (the tests change no parameter)"""
    key = (K, V, dtype)
    if key in _ENGINES:
        return _ENGINES[key]
    m = build(K, 8, dtype, V=V)
    pair = (engine(m, dtype), m)
    if keep:
        _ENGINES[key] = pair
    return pair


def phi64(m):
    with torch.no_grad():
        return m.constrained()["phi"].double()


def mixed_totals(n):
    """0, 1, 3, 64, 65 and 1000 within one call; row 0 has 1000 tokens, so one row already spans every lane pass"""
    return torch.tensor([TOTALS[(i + 5) % 6] for i in range(n)], dtype=torch.int32)


def thetas(S, n, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(S, n, K, generator=g, dtype=torch.float64), -1).to(dtype)


def bounds(theta, phi, totals, u, margin):
    """(lower, upper, ambiguous share) of the definition in float64, on the device of its arguments"""
    p = theta.double() @ phi
    c = p.cumsum(-1).contiguous()
    V, tot = c.shape[-1], c[..., -1:]
    x = u * tot
    valid = (torch.arange(u.shape[-1], device=u.device)[None, None, :] < totals[None, :, None]).expand_as(u)
    w_lo = torch.searchsorted(c, (x - margin * tot).contiguous(), right=True).clamp(max=V - 1)     # the smallest v with y < c[v]
    w_hi = torch.searchsorted(c, (x + margin * tot).contiguous(), right=True).clamp(max=V - 1)
    amb = valid & (w_lo != w_hi)
    sure = valid & (w_lo == w_hi)
    lower = torch.zeros_like(c).scatter_add_(-1, w_lo, sure.double())
    span = torch.zeros(*c.shape[:-1], V + 1, dtype=torch.float64, device=c.device)
    span.scatter_add_(-1, w_lo, amb.double()).scatter_add_(-1, w_hi + 1, -amb.double())
    upper = lower + span.cumsum(-1)[..., :V]
    return lower, upper, float(amb.sum()) / max(1.0, float(valid.sum()))


def check_counts_call(eng, m, S, n, dtype, seed):
    K, V = eng.K, eng.V
    theta = dev(thetas(S, n, K, dtype, seed), eng)
    totals = mixed_totals(n).to(eng.device)
    tmax = int(totals.max())
    u = torch.rand(S, n, tmax, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).to(eng.device)
    out = eng.sample_counts(theta, totals, u=u)
    assert out.shape == (S, n, V) and out.dtype == torch.int32
    lower, upper, share = bounds(theta, phi64(m).to(eng.device), totals, u, MARGIN[dtype])
    print(f"K={K} V={V} n={n} S={S} {dtype}: ambiguous share {share:.3e}")
    assert share <= 0.10, share
    assert torch.equal(out.sum(-1), totals[None].expand(S, n).to(torch.int64))
    o = out.double()
    assert bool((o >= lower).all()) and bool((o <= upper).all()), (float((lower - o).max()), float((o - upper).max()))
    return share


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", KS)
def test_injected_uniforms_and_theta_against_the_restatement(K, dtype):
    worst = 0.0
    for V in VS:
        eng, m = eng_for(K, V, dtype, keep=False)
        for n in NS:
            for S in SS:
                worst = max(worst, check_counts_call(eng, m, S, n, dtype, 100 * V + 10 * n + S))
    if dtype == torch.float64:
        assert worst < 1e-6            # the bound is an exact comparison there


def test_the_largest_vocabulary():
    from gdrf_amd.engine import SAMPLE_COUNTS_MAX_V
    K, n, S, V = 2, 3, 2, SAMPLE_COUNTS_MAX_V
    eng, m = eng_for(K, V, torch.float64, keep=False)
    theta = dev(thetas(S, n, K, torch.float64, 5), eng)
    totals = torch.full((n,), 100, dtype=torch.int32, device=eng.device)
    u = torch.rand(S, n, 100, generator=torch.Generator().manual_seed(6), dtype=torch.float64).to(eng.device)
    out = eng.sample_counts(theta, totals, u=u)
    lower, upper, share = bounds(theta, phi64(m).to(eng.device), totals, u, MARGIN[torch.float64])
    print("ambiguous share", share)
    assert share <= 0.10
    assert torch.equal(out.sum(-1), totals[None].expand(S, n).to(torch.int64))
    assert bool((out.double() >= lower).all()) and bool((out.double() <= upper).all())
    # mode 1 makes the draws of mode 0
    ws = dev(m.ws[:n], eng, torch.int32)
    a = eng.sample_counts(theta, totals, seed=9)
    _, zeros = eng.sample_counts(theta, totals, 1, ws=ws, seed=9)
    assert torch.equal(zeros, (a == 0).sum(1))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,V,n,S", [(5, 9, 63, 7), (128, 257, 257, 2), (2, 65, 1, 1)])
def test_philox_draws_equal_their_own_injection_bitwise(K, V, n, S, dtype):
    eng, m = eng_for(K, V, dtype)
    theta = dev(thetas(S, n, K, dtype, 3), eng)
    totals = mixed_totals(n).to(eng.device)
    ws = dev(torch.randint(0, 5, (n, V), generator=torch.Generator().manual_seed(2), dtype=torch.int32), eng, torch.int32)
    seed = 0x1234ABCD5678
    for off in (0, 1000):
        U = eng.fill_token_uniforms(seed, S, off, n, int(totals.max()))
        assert U.shape == (S, n, 1000) and U.dtype == torch.float64 and bool(((U > 0) & (U < 1)).all())
        assert torch.equal(eng.sample_counts(theta, totals, seed=seed, row_offset=off), eng.sample_counts(theta, totals, u=U))
        da, za = eng.sample_counts(theta, totals, 1, ws=ws, seed=seed, row_offset=off)
        db, zb = eng.sample_counts(theta, totals, 1, ws=ws, u=U)
        assert torch.equal(za, zb) and torch.equal(da, db)
    assert not torch.equal(eng.fill_token_uniforms(seed, S, 0, n, 8), eng.fill_token_uniforms(seed, S, 1000, n, 8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_counts_do_not_depend_on_how_the_rows_are_batched_nor_on_the_call(dtype):
    K, V, n, S, a = 5, 9, 257, 7, 100
    eng, m = eng_for(K, V, dtype)
    theta = dev(thetas(S, n, K, dtype, 4), eng)
    totals = mixed_totals(n).to(eng.device)
    one = eng.sample_counts(theta, totals, seed=11)
    two = torch.cat([eng.sample_counts(theta[:, :a].contiguous(), totals[:a], seed=11),
                     eng.sample_counts(theta[:, a:].contiguous(), totals[a:], seed=11, row_offset=a)], dim=1)
    assert torch.equal(one, two)
    assert torch.equal(one, eng.sample_counts(theta, totals, seed=11))
    assert not torch.equal(one, eng.sample_counts(theta, totals, seed=12))


def test_token_draws_are_not_the_draws_of_theta_under_the_same_seed():
    """fill_eps's normal at (row, k = j, step = s) is Box-Muller of the first two words of the Philox block with counter (row, j, s); the
    token block j of (row, sample s) must be another block: no entry of the two may agree.  Independent draws come within 1e-9 of each
    other with probability about 1e-7 over these entries; the same block would agree to a few ulps."""
    K, n, S = 5, 16, 3
    eng, _ = eng_for(K, 9, torch.float64)
    for seed, off in ((0x1234ABCD5678, 0), (7, 1000)):
        U = eng.fill_token_uniforms(seed, S, off, n, 4 * K).reshape(S, n, K, 4)
        z = torch.sqrt(-2.0 * torch.log(U[..., 0])) * torch.cos(2.0 * math.pi * U[..., 1])           # (S, n, j)
        E = torch.stack([eng.fill_eps(seed, s, off, n) for s in range(S)]).transpose(1, 2)           # (S, n, k)
        gap = float((E - z).abs().min())
        print("closest pair", gap)
        assert gap > 1e-9


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pooled_word_frequencies_follow_p(dtype):
    K, V, n, S, T = 5, 9, 64, 8, 1000
    eng, m = eng_for(K, V, dtype)
    row = thetas(1, 1, K, dtype, 21)
    theta = dev(row.expand(S, n, K), eng)
    totals = torch.full((n,), T, dtype=torch.int32, device=eng.device)
    out = eng.sample_counts(theta, totals, seed=20240229)
    p = (row[0, 0].double() @ phi64(m))
    p = p / p.sum()
    freq = out.sum((0, 1)).double().cpu() / (S * n * T)
    z = (freq - p).abs() / torch.sqrt(p * (1 - p) / (S * n * T))
    print("z", z)
    assert S * n * T == 512000 and bool((z <= 5.0).all()), z


def deviance(w, T, q):
    """2 sum_n sum_{v: w > 0} w log(w / (T_n q_v)) per sample: w (S, n, V) or (n, V), T (n,), q (S, n, V), float64"""
    w = w.double().expand_as(q)
    t = torch.where(w > 0, w * torch.log(w.clamp(min=1) / (T.double()[None, :, None] * q)), torch.zeros_like(q))
    return 2.0 * t.sum((1, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,V", [(5, 9), (128, 256), (128, 257)])
def test_check_statistics_against_the_counts_of_the_same_seed(K, V, dtype):
    n, S, a = 257, 7, 100
    eng, m = eng_for(K, V, dtype)
    theta = dev(thetas(S, n, K, dtype, 8), eng)
    g = torch.Generator().manual_seed(9)
    ws = torch.randint(0, 7, (n, V), generator=g, dtype=torch.int32)
    ws[torch.rand(n, V, generator=g) < 0.4] = 0
    ws[5] = 0                                                               # a row without tokens
    ws = ws.to(eng.device)
    totals = ws.sum(1).to(torch.int32)
    counts = eng.sample_counts(theta, totals, seed=31)
    dv, zeros = eng.sample_counts(theta, totals, 1, ws=ws, seed=31)
    assert dv.shape == (2, S) and dv.dtype == torch.float64 and zeros.shape == (S, V) and zeros.dtype == torch.int64
    assert torch.equal(zeros, (counts == 0).sum(1))
    p = theta.double() @ phi64(m).to(eng.device)
    q = p / p.sum(-1, keepdim=True)
    want_rep, want_obs = deviance(counts, totals, q), deviance(ws[None], totals, q)
    figs = dict(rep=relerr(dv[0].cpu().numpy(), want_rep.cpu().numpy()), obs=relerr(dv[1].cpu().numpy(), want_obs.cpu().numpy()))
    print(f"K={K} V={V} {dtype}", figs)
    assert figs["rep"] < TOL[dtype] and figs["obs"] < TOL[dtype], figs
    # rows cut into pieces: the integers exactly, the sums within the same tolerance
    d1, z1 = eng.sample_counts(theta[:, :a].contiguous(), totals[:a], 1, ws=ws[:a], seed=31)
    d2, z2 = eng.sample_counts(theta[:, a:].contiguous(), totals[a:], 1, ws=ws[a:], seed=31, row_offset=a)
    assert torch.equal(z1 + z2, zeros)
    assert relerr((d1 + d2).cpu().numpy(), dv.cpu().numpy()) < (1e-12 if dtype == torch.float64 else TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_surface(dtype, monkeypatch):
    import gdrf_amd.models.sparse_gdrf as sg
    K, n, S, V = 5, 257, 3, 9
    m = build(K, n, dtype, mean_function=MEAN_KN)
    big = _model(m, dtype, n, mean_function=MEAN_KN)
    xs = m.xs.to(dtype)
    totals = mixed_totals(n)
    for coherent in (False, True):
        w = big.sample_counts(xs, totals, S, seed=3, coherent=coherent)
        assert w.shape == (S, n, V) and w.dtype == torch.int32
        assert torch.equal(w.sum(-1).cpu(), totals[None].expand(S, n).to(torch.int64))
        th = big.sample_topic_maps(xs, S, seed=3) if coherent else big.sample_topic_probs(xs, S, seed=3)
        assert torch.equal(w, big.sample_counts(xs, totals, S, seed=3, theta=th))
    w = big.sample_counts(xs, totals, S, seed=3)
    assert torch.equal(big.sample_counts(xs, 64, 2), big.sample_counts(xs, torch.full((n,), 64), 2, seed=big.rng_seed))
    # rows in pieces of 80, each with its offset: the same counts and zero counts
    ws = m.ws
    chk = big.predictive_check(xs, ws, 5, seed=3)
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 80)
    assert torch.equal(w, big.sample_counts(xs, totals, S, seed=3))
    chk80 = big.predictive_check(xs, ws, 5, seed=3)
    assert torch.equal(chk["zeros_rep"], chk80["zeros_rep"]) and torch.equal(chk["zeros_obs"], chk80["zeros_obs"])
    for k in ("deviance_obs", "deviance_rep"):
        assert relerr(chk80[k].cpu().numpy(), chk[k].cpu().numpy()) < (1e-12 if dtype == torch.float64 else TOL[dtype])
    # a restored snapshot offers the same methods; a custom link runs with torch on the mu samples, as sample_topic_probs applies it
    snap = copy.deepcopy(big)
    th = big.sample_topic_probs(xs, S, seed=3)
    assert torch.equal(snap.restore(mean_function=MEAN_KN).sample_counts(xs, totals, S, seed=3, theta=th), w)
    ws_snap = snap.sample_counts(xs, totals, S, seed=3)
    assert ws_snap.shape == (S, n, V) and torch.equal(ws_snap.sum(-1).cpu(), totals[None].expand(S, n).to(torch.int64))
    assert set(snap.predictive_check(xs, ws, 4, seed=3)) == set(chk)
    linked = _model(m, dtype, 80, link_function=lambda mu: torch.softmax(mu, -2), mean_function=MEAN_KN)
    for coherent in (False, True):
        th = linked.sample_topic_maps(xs, S, seed=3) if coherent else linked.sample_topic_probs(xs, S, seed=3)
        assert torch.equal(linked.sample_counts(xs, totals, S, seed=3, coherent=coherent), linked.sample_counts(xs, totals, S, seed=3, theta=th))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_predictive_check_of_the_models_own_data(dtype):
    """Keys, shapes and ranges; and data drawn from the model are not rejected by it.  The check sets ws against replicates under EVERY
    posterior draw q_s, so data drawn under one draw are typical only of a model whose posterior is concentrated, as it is after
    training on them: the kernel variance is set to 1e-4 here (f_var, the scale of mu, is then below 0.01 everywhere) and the
    mean_function gives the rows different proportions.  p_deviance is then uniform on (0, 1) over data sets: one fixed data set."""
    K, n, S, V = 5, 257, 100, 9
    m = build(K, n, dtype, mean_function=MEAN_KN)
    with torch.no_grad():
        m.params["log_variance"].fill_(math.log(1e-4))
    model = _model(m, dtype, n, mean_function=MEAN_KN)
    xs = m.xs.to(dtype)
    totals = torch.full((n,), 200)
    ws = model.sample_counts(xs, totals, 1, seed=41)[0]
    out = model.predictive_check(xs, ws, S, seed=42)
    assert set(out) == {"deviance_obs", "deviance_rep", "p_deviance", "zeros_obs", "zeros_rep", "p_zeros"}
    assert out["deviance_obs"].shape == (S,) and out["deviance_rep"].shape == (S,) and out["p_deviance"].dim() == 0
    assert out["zeros_obs"].shape == (V,) and out["zeros_rep"].shape == (S, V) and out["p_zeros"].shape == (V,)
    assert torch.equal(out["zeros_obs"], (ws == 0).sum(0))
    p = float(out["p_deviance"])
    print("p_deviance", p, "deviance_obs", float(out["deviance_obs"].mean()), "deviance_rep", float(out["deviance_rep"].mean()),
          "p_zeros", out["p_zeros"].cpu().numpy())
    assert bool(((out["p_zeros"] >= 0) & (out["p_zeros"] <= 1)).all()) and 0.0 <= p <= 1.0
    assert float(out["deviance_rep"].min()) > 0 and float(out["deviance_obs"].min()) > 0
    assert 0.02 < p < 0.98, p


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_step_is_bitwise_the_same_after_sample_counts(dtype):
    """the call overwrites the context's Phi workspace and partial-sum scratch: a step recomputes both"""
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
    theta = dev(thetas(3, 40, K, dtype, 2), eng)
    totals = torch.full((40,), 50, dtype=torch.int32, device=eng.device)
    eng.sample_counts(theta, totals, seed=1)
    eng.sample_counts(theta, totals, 1, ws=ws[:40].contiguous(), seed=1)
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)


def test_limits():
    eng, m = eng_for(5, 9, torch.float64)
    theta = dev(thetas(2, 4, 5, torch.float64, 1), eng)
    totals = torch.full((4,), 10, dtype=torch.int32, device=eng.device)
    with pytest.raises(ValueError, match="seed"):
        eng.sample_counts(theta, totals)
    with pytest.raises(ValueError, match="contiguous"):
        eng.sample_counts(theta.float(), totals, seed=1)
    with pytest.raises(ValueError, match="contiguous"):
        eng.sample_counts(theta, totals.long(), seed=1)
    zero = eng.sample_counts(theta, torch.zeros_like(totals), seed=1)          # rows without tokens: zeros, with or without u
    assert zero.shape == (2, 4, 9) and int(zero.abs().sum()) == 0
    assert int(eng.sample_counts(theta, torch.zeros_like(totals), u=torch.zeros(2, 4, 0, dtype=torch.float64, device=eng.device)).abs().sum()) == 0
