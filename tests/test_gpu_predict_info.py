"""GPU tests of the entropy and information-gain maps (gdrf_predict_info, csrc/predict_info.h) against the float64 restatement of
tests/_info_ref.py, on the model of tests/test_gpu_predict_mc.py (grid model M = 20, variance 25, perturbed u_loc / phi_unc, contracted
u_scale_tril; float32 contexts at float32-valued parameters and the same jitter level).

Tolerances are the predictive path's (1e-9 in fp64 contexts, 5e-4 in float32 ones): the four entropies as max-abs error over max-abs
value, the two information values - differences of entropies - as max-abs error over the largest entropy of the same family in the case.
"""
import math

import pytest
import torch

from gdrf_amd.engine import INFO_NAMES, INFO_V_CHUNK
from tests._info_ref import NAMES, TOL, entropy, errors, info_ref
from tests._util import dev, relerr
from tests._mc_util import MEAN_KN, _model, build, engine

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
NS, SS = (1, 63, 257), (1, 2, 7, 64)
KS = (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128)              # both sides of every lane-group form
C = INFO_V_CHUNK
T_ENT, T_INF, W_ENT, W_INF = 0, 2, 3, 5


def check(eng, m, xs, eps, tol, mean=None):
    """all six outputs with injected eps against the restatement"""
    S, K, n = eps.shape
    ref = info_ref(m, xs, eps)
    out = eng.predict_info(dev(xs, eng), S, eps=dev(eps, eng), mean=mean)
    assert out.shape == (6, n) and out.dtype == torch.float64
    ent, inf = errors(out, ref, one_word=m.V == 1)
    print(f"K={K} V={m.V} n={n} S={S} {eng.dtype} entropies {ent:.2e} information {inf:.2e}")
    assert ent < tol and inf < tol, (ent, inf)
    return out, ref


def test_names_and_chunk_width_match_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gdrf_hip.h")).read()
    assert INFO_NAMES == NAMES
    assert int(re.search(r"#define GDRF_INFO_V_CHUNK (\d+)", header).group(1)) == INFO_V_CHUNK


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", KS)
def test_injected_eps_parity_every_form_and_shape(K, dtype):
    m = build(K, max(NS), dtype)
    eng = engine(m, dtype)
    g = torch.Generator().manual_seed(7)
    for n in NS:
        for S in SS:
            eps = torch.randn(S, K, n, generator=g, dtype=torch.float64).to(dtype)
            check(eng, m, m.xs[:n].contiguous(), eps, TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,V", [(5, 1), (5, C - 1), (5, C), (5, C + 1), (5, 2 * C + 3), (128, C + 1)])
def test_injected_eps_parity_at_the_chunk_edges(K, V, dtype):
    n, S = 63, 7
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    check(eng, m, m.xs, eps, TOL[dtype])                # V = 1: the word rows are exactly 0, held absolutely (tests/_info_ref.py::errors)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["mean_function", "unwhitened", "matern52"])
def test_injected_eps_parity_mean_unwhitened_and_matern(variant, dtype):
    mean_fn = MEAN_KN if variant == "mean_function" else None
    m = build(5, 63, dtype, kind="matern52" if variant == "matern52" else "rbf", whiten=variant != "unwhitened", mean_function=mean_fn)
    eng = engine(m, dtype)
    eps = torch.randn(7, 5, 63, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype)
    check(eng, m, m.xs, eps, TOL[dtype], mean=None if mean_fn is None else dev(mean_fn(m.xs), eng))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_eps_is_the_plug_in_and_carries_no_information(dtype):
    K, n, S = 5, 257, 3
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs = dev(m.xs, eng)
    out = eng.predict_info(xs, S, eps=torch.zeros(S, K, n, dtype=dtype, device=eng.device)).cpu()
    ht, hw = entropy(eng.predict(xs, 1).cpu()), entropy(eng.predict(xs, 2).cpu())
    figs = dict(topic=relerr(out[T_ENT].numpy(), ht.numpy()), word=relerr(out[W_ENT].numpy(), hw.numpy()),
                topic_information=float(out[T_INF].abs().max()) / float(ht.max()), word_information=float(out[W_INF].abs().max()) / float(hw.max()))
    print(dtype, {k: f"{v:.2e}" for k, v in figs.items()})
    assert all(v < TOL[dtype] for v in figs.values()), figs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_uniform_phi_hides_the_field_from_the_words(dtype):
    K, n, S = 5, 63, 64
    m = build(K, n, dtype)
    with torch.no_grad():
        m.params["phi_unc"].zero_()
    eng = engine(m, dtype)
    out = eng.predict_info(dev(m.xs, eng), S, seed=3).cpu()
    log_v = math.log(m.V)
    figs = dict(word_entropy=float((out[W_ENT] - log_v).abs().max()) / log_v, word_information=float(out[W_INF].abs().max()) / log_v,
                least_topic_information=float(out[T_INF].min()))
    print(dtype, {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["word_entropy"] < TOL[dtype] and figs["word_information"] < TOL[dtype], figs
    assert figs["least_topic_information"] > 1e-2, figs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_topic_has_no_topic_uncertainty(dtype):
    m = build(1, 63, dtype)
    eng = engine(m, dtype)
    out = eng.predict_info(dev(m.xs, eng), 7, seed=3).cpu()
    assert torch.equal(out[:3], torch.zeros(3, 63, dtype=torch.float64))
    assert float(out[W_ENT].min()) > 0.1 and float(out[W_INF].abs().max()) < TOL[dtype] * float(out[W_ENT].max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,S", [(5, 64), (2, 64), (17, 7), (128, 2)])
def test_invariants_on_free_running_draws(K, S, dtype):
    n, seed = 257, 20240229
    m = build(K, n, dtype)
    eng = engine(m, dtype)
    xs = dev(m.xs, eng)
    out = eng.predict_info(xs, S, seed=seed).cpu()
    tol_t, tol_w = TOL[dtype] * float(out[0:2].max()), TOL[dtype] * float(out[3:5].max())
    print(f"K={K} S={S} {dtype} word_information [{float(out[W_INF].min()):.3e}, {float(out[W_INF].max()):.3e}] topic_information "
          f"[{float(out[T_INF].min()):.3e}, {float(out[T_INF].max()):.3e}] least gap {float((out[T_INF] - out[W_INF]).min()):.3e}")
    assert bool((out[W_INF] >= -tol_w).all())
    assert bool((out[W_INF] <= out[T_INF] + max(tol_t, tol_w)).all())
    assert bool((out[T_INF] <= math.log(min(K, S)) + tol_t).all())
    # the same draws as predict_mc's: theta_bar is the mean its mode 1 returns
    want = entropy(eng.predict_mc(xs, 1, S, seed=seed)[0].cpu())
    assert relerr(out[T_ENT].numpy(), want.numpy()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,n,S,off,V", [(5, 63, 7, 1000, 9), (128, 257, 2, 2 ** 33 + 5, 9), (2, 1, 64, 0, 9), (9, 63, 3, 7, C + 3)])
def test_philox_draws_equal_their_own_injection_bitwise(K, n, S, off, V, dtype):
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs = dev(m.xs, eng)
    seed = 0x1234ABCD5678
    E = torch.stack([eng.fill_eps(seed, s, off, n) for s in range(S)]).contiguous()
    assert torch.equal(eng.predict_info(xs, S, seed=seed, row_offset=off), eng.predict_info(xs, S, eps=E))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [9, C + 3])
def test_results_do_not_depend_on_how_the_rows_are_batched(V, dtype):
    K, n, S = 5, 257, 7
    m = build(K, n, dtype, V=V)
    eng = engine(m, dtype)
    xs = dev(m.xs, eng)
    one = eng.predict_info(xs, S, seed=11)
    cuts = (0, 1, 101, 257)
    pieces = torch.cat([eng.predict_info(xs[a:b].contiguous(), S, seed=11, row_offset=a) for a, b in zip(cuts[:-1], cuts[1:])], dim=1)
    assert torch.equal(one, pieces)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_surface_cuts_rows_into_pieces_without_changing_the_result(dtype, monkeypatch):
    import copy

    import gdrf_amd.models.sparse_gdrf as sg
    K, n, S = 5, 257, 7
    m = build(K, n, dtype, mean_function=MEAN_KN)
    xs = m.xs.to(dtype)
    big = _model(m, dtype, n, mean_function=MEAN_KN)
    whole = big.information(xs, S, seed=3)
    assert big._engine.n_cap == n and tuple(whole) == NAMES
    assert all(v.shape == (n,) and v.dtype == torch.float64 for v in whole.values())
    monkeypatch.setattr(sg, "MC_PIECE_ROWS", 64)
    small = _model(m, dtype, 64, mean_function=MEAN_KN)
    cut = small.information(xs, S, seed=3)
    assert small._engine.n_cap == 64
    for name in NAMES:
        assert torch.equal(whole[name], cut[name]), name
    # seed=None is the model's rng_seed; against the restatement, with the mean_function, through injected draws cut into the same pieces
    assert torch.equal(small.information(xs, 2)["word_information"], small.information(xs, 2, seed=small.rng_seed)["word_information"])
    eps = torch.randn(S, K, n, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype)
    m.force_jitter_level = small._engine.last_jitter_level
    got = small.information(xs, S, eps=eps)
    ent, inf = errors(torch.stack([got[k] for k in NAMES]), info_ref(m, m.xs, eps))
    print(dtype, f"entropies {ent:.2e} information {inf:.2e}")
    assert ent < TOL[dtype] and inf < TOL[dtype]
    # a restored snapshot offers the same methods
    snap = copy.deepcopy(big)
    again = snap.restore(mean_function=MEAN_KN).information(xs, S, seed=3)
    assert relerr(again["word_information"].cpu().numpy(), whole["word_information"].cpu().numpy()) < TOL[dtype]
    linked = _model(m, dtype, 64, link_function=lambda mu: torch.softmax(mu, -2), mean_function=MEAN_KN)
    with pytest.raises(NotImplementedError):
        linked.information(xs, S)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_step_is_bitwise_the_same_after_predict_info(dtype):
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
    eng.predict_info(xs[:40].contiguous(), 3, seed=1, mean=dev(torch.ones(40), eng))
    out2, g2 = step()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)


@pytest.mark.parametrize("criterion", ["word_information", "topic_entropy"])
def test_most_informative_is_the_stable_descending_sort(criterion):
    dtype, K, n, S = torch.float64, 5, 63, 7
    m = build(K, n, dtype)
    model = _model(m, dtype, n)
    xs = m.xs.to(dtype)
    scores = model.information(xs, S, seed=3)[criterion]
    idx, top = model.most_informative(xs, n, criterion, S, seed=3)
    want = torch.sort(scores, descending=True, stable=True).indices
    assert idx.shape == (n,) and torch.equal(idx, want) and torch.equal(top, scores[want])
    idx4, top4 = model.most_informative(xs, 4, criterion, S, seed=3)
    assert torch.equal(idx4, want[:4]) and torch.equal(top4, scores[want[:4]]) and bool((top4[:-1] >= top4[1:]).all())
    with pytest.raises(ValueError, match="count"):
        model.most_informative(xs, n + 1, criterion, S)
    with pytest.raises(ValueError, match="criterion"):
        model.most_informative(xs, 4, "entropy", S)


def test_most_informative_ranks_identical_rows_in_index_order():
    """The draws are keyed by the row, so two rows at the same x score alike only where the score does not depend on the draws: with one
    topic theta = 1 in every draw, and the topic scores of all rows (two of them at the same x among them) are the same number, 0."""
    dtype, n, S = torch.float64, 63, 7
    m = build(1, n, dtype)
    with torch.no_grad():
        m.xs[9] = m.xs[5]
    model = _model(m, dtype, n)
    xs = m.xs.to(dtype)
    scores = model.information(xs, S, seed=3)
    assert torch.equal(scores["topic_information"][5], scores["topic_information"][9])
    idx, top = model.most_informative(xs, 12, "topic_information", S, seed=3)
    assert torch.equal(idx.cpu(), torch.arange(12)) and torch.equal(top.cpu(), torch.zeros(12, dtype=torch.float64))
    idx, _ = model.most_informative(xs, n, "word_entropy", S, seed=3)       # one Phi row for every x: equal again
    assert idx.tolist().index(5) < idx.tolist().index(9)
