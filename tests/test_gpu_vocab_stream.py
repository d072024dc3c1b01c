"""GPU tests of the vocabulary-streamed row form (gdrf_set_rows_form(ctx, 1), Engine(rows_form="streamed"), csrc/rows_vstream.h).

Form 1 keeps only the theta of a 64-row block in LDS and streams Phi through it in tiles of VT words (64 for float, 32 for double), so it
serves vocabularies the LDS forms reject.  It is checked against the fp64 reference where only it runs, against the LDS forms where both
run, at the edges of its tiles and grid, past 2^31 count elements, and through the model surface."""
import gc

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import RefShapedGDRF
from tests._util import dev, load_params, make_oracle, relerr
from tests.test_gpu_parity import TOL
from tests.test_gpu_rows import _aux, _assert_close, _loud_oracle

pytestmark = pytest.mark.gpu

LOSS_TOL_VS_TORCH = 1e-6          # torch evaluates lgamma(int32 counts) in float32 (tests/test_gpu_parity.py)
VT = {torch.float64: 32, torch.float32: 64}


def _engine(m, rows_form="streamed", dtype=None, n_cap=None, learn_inducing=None, ard=False):
    """Engine holding the oracle's parameters, inducing points and Dirichlet prior, in the requested row form."""
    from gdrf_amd.engine import Engine
    dtype = m.dtype if dtype is None else dtype
    learn = bool(getattr(m, "learn_inducing", False)) if learn_inducing is None else learn_inducing
    eng = Engine(n_cap or m.N, m.M, m.K, m.V, m.D, dtype=dtype, kernel=m.kind, jitter=m.jitter, maxjitter=m.maxjitter,
                 process_group=None, learn_inducing=learn, whiten=bool(getattr(m, "whiten", True)), ard=ard, rows_form=rows_form)
    assert eng.rows_form == rows_form
    eng.set_inducing_points(m.Z)
    eng.set_dirichlet(m.alpha)
    load_params(eng, m)
    return eng


def _step(eng, m, eps, **kw):
    eng.loss_and_grads(dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), **kw)
    out = eng.read_out()
    assert out["chol_failed"] == 0
    n = m.N
    rows = {name: eng.workspace(name, n).cpu().double().numpy() for name in ("q", "mu", "vbar", "locbar", "asum")}
    grads = {name: v.cpu().double().numpy() for name, v in eng.named_views(eng.grads).items()}
    return out["loss"], rows, grads


def _vs_oracle(m, eps, eng, loss, grads, tl=LOSS_TOL_VS_TORCH, tg=1e-7):
    m.force_jitter_level = eng.last_jitter_level
    loss_ref, grads_ref = m.loss_and_grads(eps)
    assert abs(loss - loss_ref) <= tl * abs(loss_ref), (loss, loss_ref)
    for name in eng.PARAM_NAMES:
        assert relerr(grads[name], grads_ref[name].numpy()) < tg, name


# ---- 1. the shape the default selection rejects (tests/test_gpu_round2.py pins its "too large") trains in form 1
def test_pinned_oversize_shape_trains_streamed():
    from gdrf_amd import _lib
    m, eps = make_oracle(dtype=torch.float64, jitter=1e-6, W=6, H=5, V=2500, K=5, n_points=(3, 2))
    eng0 = _engine(m, rows_form="auto")
    with pytest.raises(_lib.GdrfHipError, match="too large"):
        eng0.loss_and_grads(dev(m.xs, eng0), dev(m.ws, eng0, torch.int32), dev(eps, eng0))
    del eng0
    eng = _engine(m)
    loss, _, grads = _step(eng, m, eps)
    _vs_oracle(m, eps, eng, loss, grads)


# ---- 2. form 1 equals the LDS forms where both run: matrix-core (10, 50), (32, 64); register topics (5, 300); K > 32 (40, 100)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,V", [(10, 50), (32, 64), (5, 300), (40, 100)])
def test_streamed_equals_lds_forms(K, V, dtype):
    m, eps = _loud_oracle(K, V, 37, 9, dtype)
    a = _step(_engine(m, rows_form="auto"), m, eps)
    b = _step(_engine(m, rows_form="streamed"), m, eps)
    if dtype == torch.float64:
        rep = {name: relerr(b[1][name], a[1][name]) for name in a[1]}
        rep.update({"g_" + name: relerr(b[2][name], a[2][name]) for name in a[2]})
        rep["loss"] = abs(b[0] - a[0]) / abs(a[0])
        assert max(rep.values()) <= 1e-12, rep
    else:
        rows_a = {k: v for k, v in a[1].items() if k != "asum"}
        rows_b = {k: v for k, v in b[1].items() if k != "asum"}
        _assert_close(b[0], rows_b, b[2], a[0], rows_a, a[2], TOL[dtype])
        assert relerr(b[1]["asum"], a[1]["asum"]) < TOL[dtype]["w"] * 10


# ---- 3. tile and grid edges against the fp64 reference
def _clamp_word(m, v):
    """phi_kv ~ e^-40 for every topic at word v: p_v / sum p falls under eps on every row, so the clamp is active there"""
    with torch.no_grad():
        m.params["phi_unc"][:, v] = -40.0


EDGES = [(1, 1), (5, 1), (5, 31), (5, 32), (5, 33), (1, 63), (5, 64), (5, 65), (3, 2999), (128, 33), (128, 65)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,V", EDGES)
def test_streamed_tile_edges(K, V, dtype):
    # N = 37 * 9 = 333: five full 64-row blocks and a ragged one of 13 rows; the last row has 100x the counts, three rows none
    m, eps = _loud_oracle(K, V, 37, 9, dtype)
    assert m.N % 64 != 0
    clamp = V > 2 and dtype == torch.float64     # the clamp bound is the element type's epsilon: the fp64 reference clamps at fp64's
    if clamp:
        _clamp_word(m, V // 2)
    eng = _engine(m)
    loss, rows, grads = _step(eng, m, eps)
    P = {k: v.detach().double().numpy() for k, v in m.params.items()}
    loss_ref, g_ref, aux = _aux(m, eps, eng.last_jitter_level)
    _assert_close(loss, {k: rows[k] for k in ("q", "mu", "vbar", "locbar")}, grads, loss_ref, aux, g_ref, TOL[dtype])
    if clamp:
        assert P["phi_unc"][:, V // 2].max() == -40.0


def test_streamed_more_row_blocks_than_the_capped_grid():
    """K = 128, V = 4100 in fp64: 256 MiB / (K V 8) caps the grid at 63 workgroups; N = 67 * 61 = 4087 rows are 64 blocks, so one
    workgroup carries two blocks and adds the second into its Phi-bar slot."""
    K, V, dtype = 128, 4100, torch.float64
    m, eps = _loud_oracle(K, V, 67, 61, dtype)
    gcap = min(1024, max(16, (256 << 20) // (K * V * 8)), (m.N + 63) // 64)
    assert (m.N + 63) // 64 > gcap
    eng = _engine(m)
    loss, rows, grads = _step(eng, m, eps)
    loss_ref, g_ref, aux = _aux(m, eps, eng.last_jitter_level)
    _assert_close(loss, {k: rows[k] for k in ("q", "mu", "vbar", "locbar")}, grads, loss_ref, aux, g_ref, TOL[dtype])


def test_streamed_is_bit_reproducible():
    m, eps = _loud_oracle(20, 300, 37, 9, torch.float32)
    eng = _engine(m)
    a = _step(eng, m, eps)
    b = _step(eng, m, eps)
    assert a[0] == b[0]
    for name in a[2]:
        assert np.array_equal(a[2][name], b[2][name]), name


# ---- 4. every entry point past the LDS forms' ceiling (fp64, V = 1000)
V_BIG = 1000
WORLD = [(2.0, 5.0), (-1.0, 3.0)]


def _big_oracle(seed=5, K=4, **kw):
    m, eps = make_oracle(dtype=torch.float64, jitter=1e-6, W=13, H=9, V=V_BIG, K=K, n_points=(4, 3), seed=seed, **kw)
    return m, eps


@pytest.mark.parametrize("rescale", [True, False])
def test_streamed_non_unit_world(rescale):
    from gdrf_amd.data import synth_circles
    xs, ws, _ = synth_circles(17, 11, V_BIG, 3, seed=4)
    lower = torch.tensor([w[0] for w in WORLD], dtype=torch.float64)
    delta = torch.tensor([w[1] - w[0] for w in WORLD], dtype=torch.float64)
    xs_w = torch.from_numpy(xs).double() * delta + lower
    m = RefShapedGDRF(xs_w, ws, kind="rbf", K=3, n_points=(5, 4), lengthscale=0.3, dtype=torch.float64, jitter=1e-6, world=WORLD,
                      guide_rescale=rescale, optimizer="adam", lr=1e-2)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        m.params["u_loc"].add_(0.3 * torch.randn(m.params["u_loc"].shape, generator=g, dtype=torch.float64))
        m.params["phi_unc"].add_(0.5 * torch.randn(m.params["phi_unc"].shape, generator=g, dtype=torch.float64))
    eps = torch.randn(3, m.N, generator=g, dtype=torch.float64)
    loss_ref, grads_ref = m.loss_and_grads(eps)
    eng = _engine(m)
    xs_m = m.scale(xs_w)
    kw = dict(xs_guide=dev(m.scale(xs_m), eng)) if rescale else {}
    eng.loss_and_grads(dev(xs_m, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), force_level=m.last_jitter_level, **kw)
    out = eng.read_out()
    assert abs(out["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref), (out["loss"], loss_ref)
    gv = eng.named_views(eng.grads)
    for name in eng.PARAM_NAMES:
        assert relerr(gv[name].cpu().numpy(), grads_ref[name].numpy()) < 1e-7, name


@pytest.mark.parametrize("link", ["sigmoid", "tempered_softmax"])
def test_streamed_custom_link(link):
    from tests.test_gpu_round2 import _LINKS
    from gdrf_amd.data import synth_circles
    xs, ws, _ = synth_circles(17, 9, V_BIG, 4, seed=4)
    m = RefShapedGDRF(xs, ws, kind="rbf", K=4, n_points=(4, 3), lengthscale=0.2, dtype=torch.float64, jitter=1e-6,
                      link_function=_LINKS[link], optimizer="adam", lr=1e-2)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        m.params["u_loc"].add_(0.3 * torch.randn(m.params["u_loc"].shape, generator=g, dtype=torch.float64))
        m.params["phi_unc"].add_(0.5 * torch.randn(m.params["phi_unc"].shape, generator=g, dtype=torch.float64))
    eps = torch.randn(4, m.N, generator=g, dtype=torch.float64)
    eng = _engine(m)
    eng.link_function = _LINKS[link]
    loss, _, grads = _step(eng, m, eps)
    _vs_oracle(m, eps, eng, loss, grads)


def test_streamed_particles_renyi_learnable_inducing_and_predict():
    """3 particles under RenyiELBO with learnable inducing inputs, then gdrf_predict modes 0-3, against the reference."""
    m, _ = _big_oracle(learn_inducing=True, random_inducing=True)
    g = torch.Generator().manual_seed(7)
    eps = torch.randn(3, m.K, m.N, generator=g, dtype=torch.float64)
    eng = _engine(m)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    eng.loss_and_grads(xs, ws, dev(eps, eng), renyi_alpha=0.5)
    out = eng.read_out()
    m.force_jitter_level = eng.last_jitter_level
    loss_ref, grads_ref = m.loss_and_grads(eps, renyi_alpha=0.5)
    assert abs(out["loss"] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref), (out["loss"], loss_ref)
    gv = eng.named_views(eng.grads)
    for name in list(eng.PARAM_NAMES) + ["inducing_unc"]:
        assert relerr(gv[name].cpu().numpy(), grads_ref[name].numpy()) < 1e-7, name
    with torch.no_grad():
        assert relerr(eng.predict(xs, 0).cpu().numpy(), m.log_topic_probs().numpy()) < 1e-9
        assert relerr(eng.predict(xs, 1).cpu().numpy(), m.topic_probs().numpy()) < 1e-9
        assert relerr(eng.predict(xs, 2).cpu().numpy(), m.word_probs().numpy()) < 1e-9
        s = eng.predict(xs, 3, ws).cpu().numpy()
        assert abs(float(np.exp(-s[0] / s[1])) - float(m.perplexity())) < 1e-8 * float(m.perplexity())


class _Trend(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(2, 1)

    def forward(self, x):
        return self.lin(x).squeeze(-1)


def test_streamed_predict_past_n_cap():
    """gdrf_predict modes 2 and 3 take the rows n_cap at a time: 117 rows through an engine of n_cap = 50 (three chunks, the last
    ragged) against the reference"""
    m, _ = _big_oracle()
    eng = _engine(m, n_cap=50)
    xs, ws = dev(m.xs, eng), dev(m.ws, eng, torch.int32)
    assert m.N > 2 * 50
    with torch.no_grad():
        assert relerr(eng.predict(xs, 1).cpu().numpy(), m.topic_probs().numpy()) < 1e-9
        assert relerr(eng.predict(xs, 2).cpu().numpy(), m.word_probs().numpy()) < 1e-9
        s = eng.predict(xs, 3, ws).cpu().numpy()
        assert abs(float(np.exp(-s[0] / s[1])) - float(m.perplexity())) < 1e-8 * float(m.perplexity())


def test_streamed_ard_and_mean_module_through_svi():
    """ARD lengthscales, a trainable torch.nn.Module mean_function and 5 Adam steps through SVI.step: form 1 follows form 0's
    trajectory where both run (V = 60), and trains at V = 1000 where only it runs."""
    from gdrf_amd import poutine
    from gdrf_amd.data import synth_circles
    from gdrf_amd.infer import SVI, Trace_ELBO
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    from gdrf_amd.optim import Adam

    def run(V, rows_form):
        xs_np, ws_np, _ = synth_circles(14, 10, V, 3, seed=8)
        xs = torch.from_numpy(xs_np).to("cuda:0", torch.float64); ws = torch.from_numpy(ws_np).to("cuda:0")
        torch.manual_seed(0)
        mean = _Trend().double().to("cuda:0")
        model = SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2,
                                      kernel=RBF(input_dim=2, lengthscale=torch.tensor([0.2, 0.3]), variance=torch.tensor(25.0)),
                                      num_observation_categories=V, num_topic_categories=3, dirichlet_param=0.01, n_points=[4, 3],
                                      fixed_inducing_points=True, inducing_init="grid", maxjitter=15, jitter=1e-6, device="cuda:0",
                                      dtype=torch.float64, seed=3, mean_function=mean, rows_form=rows_form)
        sc = poutine.scale(scale=1.0 / xs.shape[0])
        svi = SVI(model=sc(model.model), guide=sc(model.guide), optim=Adam({"lr": 1e-2}), loss=Trace_ELBO(num_particles=1))
        g = torch.Generator().manual_seed(31)
        losses = [svi.step(xs=xs, ws=ws, subsample=False, eps=torch.randn(3, xs.shape[0], generator=g, dtype=torch.float64))
                  for _ in range(5)]
        return losses, model.state_dict()

    la, sa = run(60, "auto")
    lb, sb = run(60, "streamed")
    assert np.allclose(lb, la, rtol=1e-10, atol=0), (la, lb)
    for k in sa:
        assert relerr(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 1e-9, k
    lc, sc_ = run(V_BIG, "streamed")
    assert all(np.isfinite(lc)) and lc[-1] < lc[0], lc


@pytest.fixture
def streamed_mean_setup(monkeypatch):
    """tests/test_gpu_mean_params.py's model + oracle builder at V = 1000, its engine switched to the streamed form"""
    import tests.test_gpu_mean_params as mp
    from gdrf_amd import _lib
    orig = mp.setup

    def setup(*a, **kw):
        out = orig(*a, **kw)
        eng = out[1]._engine
        _lib.check(eng.lib.gdrf_set_rows_form(eng.ctx, 1), "gdrf_set_rows_form")
        assert eng.rows_form == "streamed" and eng.V == V_BIG
        return out

    monkeypatch.setattr(mp, "V", V_BIG)
    monkeypatch.setattr(mp, "setup", setup)
    return mp


@pytest.mark.parametrize("case", ["ard", "world", "particles"])
def test_streamed_mean_module_gradient(streamed_mean_setup, case):
    """the gradient of a torch.nn.Module mean's parameters (and every other block) against autograd through the reference"""
    kw = dict(ard=dict(ard=True), world=dict(world=True), particles=dict(P=3, renyi=0.5))[case]
    got, ref, gmax = streamed_mean_setup.check_step(mean="trend_kn", **kw)["w"]
    assert float(ref.abs().max()) > 1e-4 * gmax


def test_streamed_five_adam_steps_through_svi(streamed_mean_setup):
    """five SVI.step calls with Adam follow the oracle's trajectory, the module mean's parameters included"""
    streamed_mean_setup.test_five_steps_follow_torch_optimizers_on_the_module("adam")


def test_streamed_mean_function_gradient_against_the_reference():
    mf = lambda x: 1.5 * x[:, 0] - 0.7 * x[:, 1]
    m, eps = _big_oracle(mean_function=mf)
    eng = _engine(m)
    loss, _, grads = _step(eng, m, eps, mean=dev(mf(m.xs), eng))
    _vs_oracle(m, eps, eng, loss, grads)


# ---- 5. 64-bit offsets: n x V > 2^31 count elements
def test_streamed_offsets_past_2g_elements():
    K, V, M, n = 4, 4096, 12, 530_000
    assert n * V > 2 ** 31 and (n // 2) * V < 2 ** 31
    free, _ = torch.cuda.mem_get_info(0)
    need = n * V * 4 + n * 32 * 8 * 3 + 20 * K * n * 4 + (2 << 30)
    if free < need:
        pytest.skip(f"needs ~{need / 1e9:.1f} GB of device memory, {free / 1e9:.1f} GB free")
    m, _ = make_oracle(dtype=torch.float32, jitter=1e-4, W=8, H=6, V=V, K=K, n_points=(4, 3), perturb=False)
    from gdrf_amd.engine import Engine
    eng = Engine(n, m.M, K, V, m.D, dtype=torch.float32, kernel=m.kind, jitter=m.jitter, maxjitter=m.maxjitter, process_group=None,
                 rows_form="streamed")
    eng.set_inducing_points(m.Z); eng.set_dirichlet(m.alpha); load_params(eng, m)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    xs = torch.rand(n, 2, generator=g, device="cuda:0")
    ws = torch.randint(0, 4, (n, V), generator=g, device="cuda:0", dtype=torch.int32)
    ws[-64:, -17:] = 1_000_000                  # the last rows (past 2^31 elements) are loud
    eps = torch.randn(K, n, generator=g, device="cuda:0")
    lay = eng.red_layout

    def payload(lo, hi):
        eng.loss_and_grads(xs[lo:hi], ws[lo:hi], eps[:, lo:hi].contiguous(), n_global=n, force_level=0)
        torch.cuda.synchronize()
        return eng.red_T[lay["phibar"]:lay["A"]].double().cpu().numpy().copy(), eng.red_d[:4].cpu().numpy().copy()

    full = payload(0, n)
    h = n // 2
    a, b = payload(0, h), payload(h, n)
    assert relerr(full[0], a[0] + b[0]) < 1e-5
    assert relerr(full[1], a[1] + b[1]) < 1e-5
    # the loud rows dominate the half that holds them: a wrapped offset would have read other rows
    assert np.abs(b[0]).max() > 10 * np.abs(a[0]).max()
    del eng, ws
    gc.collect()
    torch.cuda.empty_cache()


# ---- 6. the surface
def test_rows_form_survives_snapshot_restore_and_train():
    import copy
    from gdrf_amd.data import synth_circles
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    from gdrf_amd.train import train
    xs_np, ws_np, _ = synth_circles(10, 8, V_BIG, 3, seed=2)
    xs = torch.from_numpy(xs_np).to("cuda:0"); ws = torch.from_numpy(ws_np).to("cuda:0")
    kern = RBF(input_dim=2, lengthscale=torch.tensor(0.2), variance=torch.tensor(25.0))
    model = SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2, kernel=kern, num_observation_categories=V_BIG,
                                  num_topic_categories=3, dirichlet_param=0.01, n_points=[4, 3], device="cuda:0", rows_form="streamed")
    assert model._engine.rows_form == "streamed"
    snap = copy.deepcopy(model)
    assert snap.meta["rows_form"] == "streamed"
    sd = snap.state_dict()
    restored = snap.restore()
    assert restored._engine.rows_form == "streamed"
    restored.load_state_dict(sd)
    assert np.allclose(restored.topic_probs(xs).cpu().numpy(), model.topic_probs(xs).cpu().numpy(), rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2, kernel=kern, num_observation_categories=V_BIG,
                              num_topic_categories=3, dirichlet_param=0.01, n_points=[4, 3], device="cuda:0", rows_form="tiled")
    res = train(xs=xs_np, ws=ws_np, dimensions=2, epochs=3, num_topics=3, num_inducing_points=[4, 3], rows_form="streamed")
    assert res is not None


def test_engine_rejects_an_unknown_rows_form():
    from gdrf_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine(64, 12, 3, 9, 2, process_group=None, rows_form="lds")
    assert Engine(64, 12, 3, 9, 2, process_group=None).rows_form == "auto"
