"""CPU tests of how the model's predictive methods cut their rows into pieces: every public method that serves more rows than one engine
call holds is driven on a stub (a model cannot be built without a HIP device) whose engine records each call it receives and returns
tensors whose entries along the row axis are the global row index.  With pieces of 3 rows and n in (1, 3, 4, 7) - less than a piece,
exactly one, one plus a one-row tail, several plus a tail - a test asserts the whole trace (rows, row_offset, seed, shape and contiguity
of eps / mean / u / theta, layout of the counts, the caller's object passed through where one piece covers everything), the size the
engine was asked to hold, and that the joined result reads arange(n) along its row axis."""
import math
import types

import pytest
import torch

from gdrf_amd.data import csr_to, to_csr
from gdrf_amd.engine import INFO_NAMES, QUANT_DOMINANT, QUANT_EXCEED, QUANT_QUANTILE, SCORE_NAMES

K, V, S, PIECE, SEED = 2, 4, 2, 3, 1234
NS = (1, 3, 4, 7)
DT = torch.float64


def rows_of(n):
    return torch.arange(n, dtype=DT)


def cuts(n, size=PIECE):
    return [(a, min(n, a + size)) for a in range(0, n, size)]


def describe(t, rows, caller=None):
    """(layout, shape, contiguous, is the caller's object, the global row index read along axis ``rows``) of a tensor argument"""
    if t is None:
        return None
    if t.layout != torch.strided:
        return ("csr", tuple(t.shape), None, t is caller, t.to_dense()[:, 0].tolist())
    lead = t.movedim(rows, 0).reshape(t.shape[rows], -1)[:, 0]
    return ("dense", tuple(t.shape), t.is_contiguous(), t is caller, lead.tolist())


class FakeEngine:
    """Engine's six row-pieced calls, with Engine's own signatures: each records what it was given and returns the rows it was given"""
    n_cap = PIECE

    def __init__(self):
        self.calls, self.caller = [], {}

    def rec(self, call, xs, **kw):
        assert xs.is_contiguous() and xs.shape[0] <= self.n_cap
        self.calls.append(dict(call=call, rows=xs[:, 0].tolist(), **kw))
        return xs[:, 0].to(DT)

    def draws(self, seed, row_offset, eps, mean):
        return dict(seed=seed, row_offset=row_offset, eps=describe(eps, 2), mean=describe(mean, 1))

    def predict_mc(self, xs, mode, num_samples, ws=None, seed=None, row_offset=0, eps=None, mean=None):
        r = self.rec("predict_mc", xs, mode=mode, S=num_samples, ws=describe(ws, 0, self.caller.get("ws")), **self.draws(seed, row_offset, eps, mean))
        m = len(r)
        if mode == 2:
            return torch.stack([r.sum(), torch.tensor(float(m), dtype=DT)])
        return {0: r[None, :, None].expand(num_samples, m, K), 1: r[None, :, None].expand(2, m, K),
                3: r[None, None, :].expand(num_samples, K, m)}[mode].clone()

    def predict_info(self, xs, num_samples, seed=None, row_offset=0, eps=None, mean=None):
        r = self.rec("predict_info", xs, S=num_samples, **self.draws(seed, row_offset, eps, mean))
        return r[None].expand(len(INFO_NAMES), len(r)).clone()

    def predict_score(self, xs, ws, num_samples, seed=None, row_offset=0, eps=None, mean=None):
        r = self.rec("predict_score", xs, S=num_samples, ws=describe(ws, 0, self.caller.get("ws")), **self.draws(seed, row_offset, eps, mean))
        return r[None].expand(len(SCORE_NAMES), len(r)).clone()

    def predict_quant(self, xs, mode, num_samples, levels=None, words=None, seed=None, row_offset=0, eps=None, mean=None):
        r = self.rec("predict_quant", xs, mode=mode, S=num_samples, levels=levels, **self.draws(seed, row_offset, eps, mean),
                     words=None if words is None else (words.dtype, words.is_contiguous(), words.tolist()))
        if mode == QUANT_DOMINANT:
            return r[:, None].expand(len(r), K).clone()
        return r[None, :, None].expand(len(levels), len(r), K if words is None else len(words)).clone()

    def fold_in(self, xs, ws, mode, num_iters=64, tol=1e-6, ws_score=None, mean=None):
        r = self.rec("fold_in", xs, mode=mode, num_iters=num_iters, tol=tol, ws=describe(ws, 0, self.caller.get("ws")),
                     ws_score=describe(ws_score, 0, self.caller.get("ws_score")), mean=describe(mean, 1))
        m = len(r)
        out = {0: r[:, None].expand(m, K), 1: r[None].expand(K, m), 2: r[:, None].expand(m, K),
               3: torch.stack([r.sum(), torch.tensor(float(m), dtype=DT)])}[mode].clone()
        return out, r[None].expand(3, m).clone()

    def sample_counts(self, theta, totals, mode=0, ws=None, seed=None, row_offset=0, u=None):
        m = theta.shape[1]
        assert totals.dtype == torch.int32 and totals.is_contiguous() and totals.shape == (m,)
        self.calls.append(dict(call="sample_counts", mode=mode, theta=describe(theta, 1, self.caller.get("theta")), totals=totals.tolist(),
                               ws=describe(ws, 0, self.caller.get("ws")), seed=seed, row_offset=row_offset, u=describe(u, 1)))
        r = theta[0, :, 0].to(DT)
        if mode == 0:
            return r[None, :, None].expand(theta.shape[0], m, V).to(torch.int32).contiguous()
        return r.sum().expand(2, theta.shape[0]).clone(), torch.full((theta.shape[0], V), m, dtype=torch.int64)


def make_stub(link=None, mean=False):
    """The model's own methods on what they read from a model: sizes, the link, the seed, device and dtype, inputs prepared as the model
    prepares them (a tensor that already has the device, dtype and layout comes back as the same object), a mean_function that returns the
    row index as a (n,) vector - so that its (K, n) expansion is not contiguous - and an engine that records."""
    from gdrf_amd.models import SparseMultinomialGDRF as G

    class Stub:
        _K, _V, M, _link_function, rng_seed, device, dtype = K, V, 6, link, SEED, torch.device("cpu"), DT

        def __init__(self):
            self.engine, self.asked = FakeEngine(), []

        def _engine_for(self, n):
            self.asked.append(n)
            return self.engine

        def _prepare_inputs(self, xs, ws=None):
            xs_s = torch.as_tensor(xs).to(self.dtype).contiguous()
            if ws is None:
                return xs_s, None
            if ws.layout != torch.strided:
                return xs_s, csr_to(ws, self.device)
            return xs_s, torch.as_tensor(ws).to(device=self.device, dtype=torch.int32).contiguous()

        def _mean_values(self, xs_s):
            return xs_s[:, 0].clone() if mean else None

        def _mean_kn(self, values, n):
            return torch.as_tensor(values).to(device=self.device, dtype=self.dtype).expand(self._K, n)

    for name, f in vars(G).items():
        if isinstance(f, types.FunctionType) and not name.startswith("__") and name not in vars(Stub):
            setattr(Stub, name, f)
    Stub.K, Stub.V = K, V
    return Stub()


@pytest.fixture(autouse=True)
def small_pieces(monkeypatch):
    from gdrf_amd.models import sparse_gdrf
    monkeypatch.setattr(sparse_gdrf, "MC_PIECE_ROWS", PIECE)


def xs_of(n):
    return rows_of(n)[:, None].expand(n, 2).contiguous()


def eps_of(n):
    return rows_of(n)[None, None, :].expand(S, K, n).contiguous()


def counts_of(n, sparse):
    ws = torch.arange(n, dtype=torch.int32)[:, None].expand(n, V).contiguous()          # every entry of row i is i
    return to_csr(ws) if sparse else ws


def sliced(n, a, b, shape, contiguous=True, layout="dense", whole_object=False):
    """what describe() gives for rows [a, b) of an argument: ``whole_object`` says that a piece covering everything passes the object"""
    return (layout, shape, None if layout == "csr" else contiguous, whole_object and (a, b) == (0, n), list(range(a, b)))


def draws(n, a, b, seed, eps, mean):
    return dict(seed=seed, row_offset=a, eps=sliced(n, a, b, (S, K, b - a)) if eps else None,
                mean=sliced(n, a, b, (K, b - a), contiguous=False) if mean else None)


def mc_trace(n, call, seed=SEED, eps=False, mean=False, **fixed):
    return [dict(call=call, rows=list(range(a, b)), **fixed, **draws(n, a, b, seed, eps, mean)) for a, b in cuts(n)]


def row_ids(t, axis):
    """assert that every fibre of ``t`` along ``axis`` is arange(n) and return n"""
    want = torch.arange(t.shape[axis], dtype=DT)
    assert torch.equal(t.to(DT).movedim(axis, -1), want.expand(t.movedim(axis, -1).shape)), t
    return t.shape[axis]


# ------------------------------------------------------------------ Engine.predict_mc
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed,eps,mean", [(None, False, False), (7, True, True)])
@pytest.mark.parametrize("linked", [False, True], ids=["softmax", "link"])
def test_sample_topic_probs_with_and_without_a_link(linked, seed, eps, mean, n):
    s = make_stub(link=staticmethod(lambda mu: mu) if linked else None, mean=mean)
    out = s.sample_topic_probs(xs_of(n), S, seed=seed, eps=eps_of(n) if eps else None)
    assert out.shape == (S, n, K) and row_ids(out, 1) == n
    assert s.asked == [min(n, PIECE)]
    assert s.engine.calls == mc_trace(n, "predict_mc", SEED if seed is None else seed, eps, mean, mode=3 if linked else 0, S=S, ws=None)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("linked", [False, True], ids=["softmax", "link"])
def test_topic_probs_mc(linked, n):
    s = make_stub(link=staticmethod(lambda mu: mu) if linked else None, mean=True)
    mean, var = s.topic_probs_mc(xs_of(n), S, seed=5)
    assert mean.shape == var.shape == (n, K) and row_ids(mean, 0) == n
    assert torch.equal(var, torch.zeros(n, K, dtype=DT)) if linked else row_ids(var, 0) == n
    assert s.asked == [min(n, PIECE)]
    assert s.engine.calls == mc_trace(n, "predict_mc", 5, mean=True, mode=3 if linked else 1, S=S, ws=None)


@pytest.mark.parametrize("n", NS)
def test_predictive_perplexity_slices_the_counts_of_every_piece_and_adds_the_sums(n):
    s, ws = make_stub(), counts_of(n, False)
    s.engine.caller["ws"] = ws
    ppl = s.predictive_perplexity(xs_of(n), ws, S)
    assert ppl.dim() == 0 and abs(float(ppl) - math.exp(-sum(range(n)) / n)) < 1e-12
    assert s.asked == [min(n, PIECE)]
    assert s.engine.calls == [dict(c, ws=sliced(n, a, b, (b - a, V))) for c, (a, b) in zip(mc_trace(n, "predict_mc", mode=2, S=S), cuts(n))]


# ------------------------------------------------------------------ Engine.predict_info
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed,eps,mean", [(None, False, False), (7, True, True)])
def test_information(seed, eps, mean, n):
    s = make_stub(mean=mean)
    d = s.information(xs_of(n), S, seed=seed, eps=eps_of(n) if eps else None)
    assert tuple(d) == INFO_NAMES and all(v.shape == (n,) and row_ids(v, 0) == n for v in d.values())
    assert s.asked == [min(n, PIECE)]
    assert s.engine.calls == mc_trace(n, "predict_info", SEED if seed is None else seed, eps, mean, S=S)


# ------------------------------------------------------------------ Engine.predict_quant
ALL_WORDS = (torch.int32, True, list(range(V)))
QUANT_CALLS = {
    "topic_quantiles": (lambda s, xs, **kw: s.topic_probs_quantiles(xs, (0.25, 0.5, 0.75), S, **kw), QUANT_QUANTILE, [0.25, 0.5, 0.75], None, K),
    "word_quantiles_all": (lambda s, xs, **kw: s.word_probs_quantiles(xs, (0.5,), None, S, **kw), QUANT_QUANTILE, [0.5], ALL_WORDS, V),
    "word_quantiles_some": (lambda s, xs, **kw: s.word_probs_quantiles(xs, (0.5,), [3, 0, 3], S, **kw), QUANT_QUANTILE, [0.5],
                            (torch.int32, True, [3, 0, 3]), 3),
    "exceedance_topic": (lambda s, xs, **kw: s.exceedance(xs, 0.5, num_samples=S, **kw), QUANT_EXCEED, [0.5], None, K),
    "exceedance_word": (lambda s, xs, **kw: s.exceedance(xs, (0.25, 2.0), "word", None, S, **kw), QUANT_EXCEED, [0.25, 2.0], ALL_WORDS, V),
}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed,eps,mean", [(None, False, False), (7, True, True)])
@pytest.mark.parametrize("name", QUANT_CALLS)
def test_the_quantile_family_joins_along_axis_one(name, seed, eps, mean, n):
    call, mode, levels, words, C = QUANT_CALLS[name]
    s = make_stub(mean=mean)
    out = call(s, xs_of(n), seed=seed, eps=eps_of(n) if eps else None)
    assert out.shape == (len(levels), n, C) and row_ids(out, 1) == n
    assert s.asked == [min(n, PIECE)]
    assert s.engine.calls == mc_trace(n, "predict_quant", SEED if seed is None else seed, eps, mean, mode=mode, S=S, levels=levels, words=words)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed,eps,mean", [(None, False, False), (7, True, True)])
def test_dominant_topic_probs_joins_along_axis_zero(seed, eps, mean, n):
    s = make_stub(mean=mean)
    out = s.dominant_topic_probs(xs_of(n), S, seed=seed, eps=eps_of(n) if eps else None)
    assert out.shape == (n, K) and row_ids(out, 0) == n
    assert s.asked == [min(n, PIECE)]
    assert s.engine.calls == mc_trace(n, "predict_quant", SEED if seed is None else seed, eps, mean, mode=QUANT_DOMINANT, S=S, levels=None, words=None)


# ------------------------------------------------------------------ Engine.predict_score
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed,eps,mean", [(None, False, False), (7, True, True)])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_pointwise_log_likelihood(sparse, seed, eps, mean, n):
    s, ws = make_stub(mean=mean), counts_of(n, sparse)
    s.engine.caller["ws"] = ws
    d = s.pointwise_log_likelihood(xs_of(n), ws, S, seed=seed, eps=eps_of(n) if eps else None)
    assert tuple(d) == SCORE_NAMES and all(v.shape == (n,) and row_ids(v, 0) == n for v in d.values())
    assert s.asked == [min(n, PIECE)]
    want = mc_trace(n, "predict_score", SEED if seed is None else seed, eps, mean, S=S)
    assert s.engine.calls == [dict(c, ws=sliced(n, a, b, (b - a, V), layout="csr" if sparse else "dense", whole_object=True))
                              for c, (a, b) in zip(want, cuts(n))]


def test_normalized_adds_the_log_coefficient_after_the_join():
    s = make_stub()
    d = s.pointwise_log_likelihood(xs_of(7), counts_of(7, False), S, normalized=True)
    assert torch.equal(d["lpd"], 2 * rows_of(7)) and torch.equal(d["mean_log_lik"], 2 * rows_of(7)) and row_ids(d["log_coef"], 0) == 7


# ------------------------------------------------------------------ Engine.fold_in
FOLD = {"infer_topic_probs": (0, 0), "infer_log_topic_probs": (1, 1), "topic_counts": (2, 0)}      # name: (mode, row axis)


def fold_trace(n, mode, sparse, mean, score):
    lay = "csr" if sparse else "dense"
    return [dict(call="fold_in", rows=list(range(a, b)), mode=mode, num_iters=9, tol=1e-3,
                 ws=sliced(n, a, b, (b - a, V), layout=lay, whole_object=True),
                 ws_score=sliced(n, a, b, (b - a, V), layout=lay, whole_object=True) if score else None,
                 mean=sliced(n, a, b, (K, b - a), contiguous=False) if mean else None) for a, b in cuts(n)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("mean", [False, True], ids=["zero_mean", "mean"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("name", FOLD)
def test_fold_in_results_and_diagnostics(name, sparse, mean, n):
    mode, axis = FOLD[name]
    s, ws = make_stub(mean=mean), counts_of(n, sparse)
    s.engine.caller["ws"] = ws
    out = getattr(s, name)(xs_of(n), ws, 9, 1e-3)
    assert out.shape == ((K, n) if mode == 1 else (n, K)) and row_ids(out, axis) == n
    assert s.asked == [min(n, PIECE)] and s.engine.calls == fold_trace(n, mode, sparse, mean, False)
    out2, diag = getattr(s, name)(xs_of(n), ws, 9, 1e-3, return_diagnostics=True)
    assert torch.equal(out2, out) and diag.shape == (3, n) and row_ids(diag, 1) == n
    assert s.asked == [min(n, PIECE)] * 2 and s.engine.calls[len(cuts(n)):] == fold_trace(n, mode, sparse, mean, False)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("mean", [False, True], ids=["zero_mean", "mean"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_completion_perplexity_adds_the_sums_of_the_pieces(sparse, mean, n):
    s, ws, sc = make_stub(mean=mean), counts_of(n, sparse), counts_of(n, sparse)
    s.engine.caller.update(ws=ws, ws_score=sc)
    ppl, diag = s.completion_perplexity(xs_of(n), ws, sc, 9, 1e-3, return_diagnostics=True)
    assert ppl.dim() == 0 and abs(float(ppl) - math.exp(-sum(range(n)) / n)) < 1e-12
    assert diag.shape == (3, n) and row_ids(diag, 1) == n
    assert s.asked == [min(n, PIECE)] and s.engine.calls == fold_trace(n, 3, sparse, mean, True)
    assert abs(float(s.completion_perplexity(xs_of(n), ws, sc, 9, 1e-3)) - float(ppl)) == 0.0


# ------------------------------------------------------------------ Engine.sample_counts
def counts_trace(n, mode, seed, theta_object, ws=False, u=False, tmax=2):
    return [dict(call="sample_counts", mode=mode, theta=sliced(n, a, b, (S, b - a, K), whole_object=theta_object),
                 totals=[i % 3 for i in range(a, b)] if not ws else [i * V for i in range(a, b)],
                 ws=sliced(n, a, b, (b - a, V)) if ws else None, seed=seed, row_offset=a,
                 u=sliced(n, a, b, (S, b - a, tmax)) if u else None) for a, b in cuts(n)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed,inject_u", [(None, False), (7, True)])
def test_sample_counts_with_injected_theta_and_u(seed, inject_u, n):
    s = make_stub()
    theta = rows_of(n)[None, :, None].expand(S, n, K).contiguous()
    u = (rows_of(n) / 16)[None, :, None].expand(S, n, 2).contiguous() if inject_u else None
    s.engine.caller["theta"] = theta
    out = s.sample_counts(xs_of(n), torch.arange(n) % 3, S, seed=seed, theta=theta, u=u)
    assert out.shape == (S, n, V) and out.dtype == torch.int32 and row_ids(out, 1) == n
    assert s.asked == [1]
    want = counts_trace(n, 0, SEED if seed is None else seed, True, u=inject_u)
    for c in s.engine.calls:
        if c["u"] is not None:
            c["u"] = c["u"][:4] + ([v * 16 for v in c["u"][4]],)
    assert s.engine.calls == want


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed", [None, 7])
def test_predictive_check_draws_theta_in_pieces_and_adds_the_statistics(seed, n):
    s, ws = make_stub(), counts_of(n, False)
    s.engine.caller["ws"] = ws
    d = s.predictive_check(xs_of(n), ws, S, seed=seed)
    total = float(sum(range(n)))
    assert torch.equal(d["deviance_rep"], torch.full((S,), total, dtype=DT)) and torch.equal(d["deviance_obs"], d["deviance_rep"])
    assert torch.equal(d["zeros_rep"], torch.full((S, V), n, dtype=torch.int64)) and torch.equal(d["zeros_obs"], torch.ones(V, dtype=torch.int64))
    assert float(d["p_deviance"]) == 1.0 and torch.equal(d["p_zeros"], torch.ones(V, dtype=DT))
    assert s.asked == [min(n, PIECE), 1]
    k = SEED if seed is None else seed
    assert s.engine.calls == mc_trace(n, "predict_mc", k, mode=0, S=S, ws=None) + counts_trace(n, 1, k, False, ws=True)


# ------------------------------------------------------------------ the piece size
def test_the_engine_calls_cut_by_n_cap_and_the_count_sampler_by_mc_piece_rows(monkeypatch):
    """MC_PIECE_ROWS = 2 under an engine that holds 3 rows: the engine is asked for min(n, 2) rows and its calls cut by the 3 it has;
    the count sampler, which holds nothing per row in the engine, cuts by 2"""
    from gdrf_amd.models import sparse_gdrf
    monkeypatch.setattr(sparse_gdrf, "MC_PIECE_ROWS", 2)
    n, ws = 7, counts_of(7, False)
    for call in (lambda s: s.sample_topic_probs(xs_of(n), S), lambda s: s.information(xs_of(n), S), lambda s: s.dominant_topic_probs(xs_of(n), S),
                 lambda s: s.pointwise_log_likelihood(xs_of(n), ws, S), lambda s: s.infer_topic_probs(xs_of(n), ws)):
        s = make_stub()
        call(s)
        assert s.asked == [2] and [c["rows"] for c in s.engine.calls] == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0]]
    s = make_stub()
    theta = rows_of(n)[None, :, None].expand(S, n, K).contiguous()
    out = s.sample_counts(xs_of(n), 1, S, theta=theta)
    assert s.asked == [1] and [c["row_offset"] for c in s.engine.calls] == [0, 2, 4, 6] and row_ids(out, 1) == n
    assert [c["theta"][4] for c in s.engine.calls] == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0], [6.0]]
