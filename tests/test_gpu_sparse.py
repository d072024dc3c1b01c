"""GPU tests of the sparse row form (a torch.sparse_csr count matrix bound with gdrf_bind_counts_csr, csrc/rows_csr.h).

The sparse form visits the stored entries only and must compute what the dense vocabulary-streamed form computes on the densified
counts, up to the order of its sums: both run in one test on identical data and are held to the bounds test_streamed_equals_lds_forms
holds the two dense forms to.  Where no dense form can run (V = 20 000 on the LDS forms, 9.2e9 count elements on any) the fp64 oracle and
known answers at initialisation are the check."""
import gc
import math

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import RefShapedGDRF
from tests._util import dev, load_params, make_oracle, relerr
from tests.test_gpu_parity import TOL
from tests.test_gpu_rows import _assert_close, _loud_oracle
from tests.test_gpu_vocab_stream import WORLD, _clamp_word, _engine, _vs_oracle

pytestmark = pytest.mark.gpu


def _thin(m, density, seed=11):
    """keep about `density` of the oracle's count entries (all of them at 1.0); the loud last row and word keep theirs"""
    if density >= 1.0:
        return
    rng = np.random.default_rng(seed)
    ws = m.ws.numpy().copy()
    keep = rng.random(ws.shape) < density
    keep[-1, :] = True
    ws[~keep] = 0
    m.ws = torch.from_numpy(ws)


def _csr(ws, eng, full=False):
    """the oracle's counts as a CSR tensor on the engine's device; full = every entry stored, zeros included"""
    from gdrf_amd.data import to_csr
    d = torch.as_tensor(ws).to(torch.int32)
    if not full:
        return to_csr(d.to(eng.device))
    n, V = d.shape
    return torch.sparse_csr_tensor(torch.arange(0, n * V + 1, V), torch.arange(V).repeat(n), d.reshape(-1), size=(n, V)).to(eng.device)


def _step(eng, m, eps, ws, **kw):
    eng.loss_and_grads(dev(m.xs, eng), ws, dev(eps, eng), **kw)
    out = eng.read_out()
    assert out["chol_failed"] == 0
    rows = {name: eng.workspace(name, m.N).cpu().double().numpy() for name in ("q", "mu", "vbar", "locbar", "asum")}
    grads = {name: v.cpu().double().numpy() for name, v in eng.named_views(eng.grads).items()}
    return out["loss"], rows, grads


def _equal(a, b, dtype):
    """b (sparse) against a (dense streamed): 1e-12 relative in fp64, TOL[float32] in fp32"""
    rep = {name: relerr(b[1][name], a[1][name]) for name in a[1]}
    rep.update({"g_" + name: relerr(b[2][name], a[2][name]) for name in a[2]})
    rep["loss"] = abs(b[0] - a[0]) / abs(a[0])
    print({k: f"{v:.2e}" for k, v in rep.items()})
    if dtype == torch.float64:
        assert max(rep.values()) <= 1e-12, rep
    else:
        rows_a = {k: v for k, v in a[1].items() if k != "asum"}
        rows_b = {k: v for k, v in b[1].items() if k != "asum"}
        _assert_close(b[0], rows_b, b[2], a[0], rows_a, a[2], TOL[dtype])
        assert relerr(b[1]["asum"], a[1]["asum"]) < TOL[dtype]["w"] * 10


def _both(m, eps, dtype, ws_sparse=None, setup=None, **kw):
    """one step of the dense streamed form and of the sparse form on the same data"""
    ea, eb = _engine(m, rows_form="streamed"), _engine(m, rows_form="auto")
    for e in (ea, eb):
        if setup:
            setup(e)
    a = _step(ea, m, eps, dev(m.ws, ea, torch.int32), **kw)
    b = _step(eb, m, eps, _csr(m.ws, eb) if ws_sparse is None else ws_sparse(eb), **kw)
    assert eb.rows_form == "auto"
    _equal(a, b, dtype)
    return a, b


# ---- 1. sparse equals dense streamed, by shape and density
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("density", [0.02, 0.3, 1.0])
@pytest.mark.parametrize("K,V", [(10, 50), (32, 64), (5, 300), (40, 100), (128, 65), (8, 50), (9, 50), (33, 64)])
def test_sparse_equals_dense_streamed(K, V, density, dtype):
    m, eps = _loud_oracle(K, V, 37, 9, dtype)
    _thin(m, density)
    _both(m, eps, dtype, ws_sparse=(lambda e: _csr(m.ws, e, full=True)) if density >= 1.0 else None)


# ---- 2. structure edges
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("full_row", [True, False])
def test_sparse_structure_edges(full_row, dtype):
    """rows with no entry, a column present in (nearly) every row of N = 67 * 13 = 871 rows (four column segments of 256), stored zeros,
    descending column indices inside every row, N not a multiple of the row block; and either a row with all V entries or (the two
    exclude each other) columns with no entry"""
    K, V = 20, 70
    m, eps = _loud_oracle(K, V, 67, 13, dtype)
    N = m.N
    assert N > 3 * 256 and N % 16 != 0
    _thin(m, 0.1)
    ws = m.ws.numpy().copy()
    empty_rows = [3, 50, N - 2]
    ws[:, 7] = np.maximum(ws[:, 7], 1)             # a word in every sample ...
    ws[empty_rows] = 0                             # ... but the samples without words
    if full_row:
        ws[5] = np.arange(1, V + 1)                # a sample with every word
    else:
        ws[:, [11, 12, V - 2]] = 0                 # words in no sample
    m.ws = torch.from_numpy(ws.astype(np.int32))
    stored = ws > 0
    stored[::9, 20] = True                         # stored zeros (word 20 is thin: most of these hold the value 0)
    stored[empty_rows] = False
    assert (ws[stored] == 0).any() and stored[:, 7].sum() == N - 3 and not stored[3].any()
    assert stored[5].all() if full_row else not stored[:, 11].any()

    def build(e):
        crow = np.concatenate([[0], np.cumsum(stored.sum(1))])
        cols = np.concatenate([np.nonzero(r)[0][::-1] for r in stored])          # descending inside a row
        vals = np.concatenate([w[np.nonzero(r)[0][::-1]] for r, w in zip(stored, ws)])
        return torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(cols), torch.from_numpy(vals.astype(np.int32)),
                                       size=(N, V)).to(e.device)
    _both(m, eps, dtype, ws_sparse=build)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N,V", [(1, 9), (333, 1)])
def test_sparse_single_row_and_single_word(N, V, dtype):
    if N == 1:                                     # the loud last row of a 2 x 2 lattice, alone
        m, eps = _loud_oracle(4, V, 2, 2, dtype)
        m.xs, m.ws, m.N, eps = m.xs[-1:], m.ws[-1:], 1, eps[:, -1:].contiguous()
    else:
        m, eps = _loud_oracle(4, V, 37, 9, dtype)
    _both(m, eps, dtype)


# ---- 3. the clamp active at a stored entry
def test_sparse_clamp_at_a_stored_entry():
    K, V, dtype = 5, 300, torch.float64
    m, eps = _loud_oracle(K, V, 37, 9, dtype)
    _thin(m, 0.3)
    ws = m.ws.numpy().copy()
    ws[:, V // 2] = 3
    m.ws = torch.from_numpy(ws)
    _clamp_word(m, V // 2)
    _both(m, eps, dtype)


# ---- 4. the other step variants
@pytest.mark.parametrize("rescale", [True, False])
def test_sparse_non_unit_world(rescale):
    from gdrf_amd.data import synth_circles
    xs, ws, _ = synth_circles(17, 11, 200, 3, seed=4)
    ws[np.random.default_rng(2).random(ws.shape) > 0.1] = 0
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
    xs_m = m.scale(xs_w)
    res = []
    for sparse in (False, True):
        eng = _engine(m, rows_form="auto" if sparse else "streamed")
        kw = dict(xs_guide=dev(m.scale(xs_m), eng)) if rescale else {}
        w = _csr(m.ws, eng) if sparse else dev(m.ws, eng, torch.int32)
        eng.loss_and_grads(dev(xs_m, eng), w, dev(eps, eng), force_level=0, **kw)
        res.append((eng.read_out()["loss"], {n: v.cpu().double().numpy() for n, v in eng.named_views(eng.grads).items()}))
    assert abs(res[1][0] - res[0][0]) <= 1e-12 * abs(res[0][0])
    for name in res[0][1]:
        assert relerr(res[1][1][name], res[0][1][name]) <= 1e-12, name


@pytest.mark.parametrize("link", ["sigmoid", "tempered_softmax"])
def test_sparse_custom_link(link):
    from tests.test_gpu_round2 import _LINKS
    m, eps = _loud_oracle(6, 120, 37, 9, torch.float64)
    _thin(m, 0.2)

    def setup(e):
        e.link_function = _LINKS[link]
    _both(m, eps, torch.float64, setup=setup)


def test_sparse_particles_renyi_and_learnable_inducing():
    m, _ = make_oracle(dtype=torch.float64, jitter=1e-6, W=13, H=9, V=150, K=4, n_points=(4, 3), seed=5, learn_inducing=True,
                       random_inducing=True)
    _thin(m, 0.15)
    g = torch.Generator().manual_seed(7)
    eps = torch.randn(3, m.K, m.N, generator=g, dtype=torch.float64)
    a, b = _both(m, eps, torch.float64, renyi_alpha=0.5)
    assert "inducing_unc" in b[2]
    _both(m, eps, torch.float64)                    # Trace_ELBO over the three particles


# ---- 5. predict mode 3, perplexity and the data constant
def test_sparse_predict_perplexity_and_ll_const_past_n_cap():
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, TOL[torch.float32]["loss"])):
        m, _ = make_oracle(dtype=dtype, jitter=1e-4 if dtype == torch.float32 else 1e-6, W=13, H=9, V=90, K=4, n_points=(4, 3), seed=5)
        _thin(m, 0.2)
        ea, eb = _engine(m, rows_form="streamed", n_cap=50), _engine(m, rows_form="auto", n_cap=50)
        assert m.N > 2 * 50
        xs = dev(m.xs, ea)
        wd, wc = dev(m.ws, ea, torch.int32), _csr(m.ws, eb)
        sa, sb = ea.predict(xs, 3, wd).cpu().numpy(), eb.predict(xs, 3, wc).cpu().numpy()
        assert relerr(sb, sa) <= tol, (sa, sb)
        assert sb[1] == float(m.ws.sum())
        la, lb = ea.ll_const(wd), eb.ll_const(wc)
        assert abs(lb - la) <= 1e-14 * abs(la), (la, lb)
        # the modes that read no counts do what they do without a binding: on the LDS forms (eb) ...
        t12 = 1e-12 if dtype == torch.float64 else 1e-4
        assert relerr(eb.predict(xs, 1).cpu().numpy(), ea.predict(xs, 1).cpu().numpy()) <= t12
        assert relerr(eb.predict(xs, 2).cpu().numpy(), ea.predict(xs, 2).cpu().numpy()) <= t12
        # ... and on a streamed engine, bit for bit, while a matrix is bound to it (its mode 2 runs the streamed kernel on dense scratch)
        ec = _engine(m, rows_form="streamed", n_cap=50)
        sc = ec.predict(xs, 3, _csr(m.ws, ec)).cpu().numpy()          # the engine's first call: none of the dense form's scratch exists yet
        assert ec._csr_bound and relerr(sc, sa) <= tol
        for mode in (0, 1, 2):
            assert torch.equal(ec.predict(xs, mode), ea.predict(xs, mode)), mode
        assert ec._csr_bound
        assert relerr(ec.predict(xs, 3, wd).cpu().numpy(), sa) == 0.0 and not ec._csr_bound


def test_model_perplexity_past_n_cap_and_under_a_custom_link():
    """model.perplexity(x, <csr>) on a model whose engine holds fewer rows than x (several n_cap pieces), against the dense value; and with
    a custom link_function, where it sums over the stored entries of the dense word_probs"""
    from gdrf_amd.data import to_csr
    from tests.test_gpu_round2 import _LINKS
    V = 90
    xs_np, ws_np = _thin_counts(14, 10, V, 3, 0.2)
    xs = torch.from_numpy(xs_np).to("cuda:0", torch.float64)
    wd = torch.from_numpy(ws_np).to("cuda:0")
    wc = to_csr(wd)
    for link in (None, "sigmoid"):
        kw = {} if link is None else dict(link_function=_LINKS[link])
        ma, _ = _model(xs[:40], wd[:40], V, rows_form="streamed", **kw)
        mb, _ = _model(xs[:40], None, V, **kw)
        assert ma._engine.n_cap == mb._engine.n_cap == 40 and len(xs) > 3 * 40
        with torch.no_grad():
            g = torch.Generator().manual_seed(3)
            u = 0.3 * torch.randn(3, ma.M, generator=g, dtype=torch.float64).to("cuda:0")
            f = 0.5 * torch.randn(3, V, generator=g, dtype=torch.float64).to("cuda:0")
            for mm in (ma, mb):
                mm._engine.view("u_loc").add_(u); mm._engine.view("phi_unc").add_(f)
        pa, pb = float(ma.perplexity(xs, wd)), float(mb.perplexity(xs, wc))
        assert mb._engine.n_cap == 40
        assert abs(pb - pa) <= 1e-12 * pa, (link, pa, pb)


def test_sparse_and_dense_calls_alternate_on_one_engine():
    """a dense ws after a CSR one clears the binding, and the reverse binds again"""
    m, eps = _loud_oracle(10, 50, 37, 9, torch.float64)
    _thin(m, 0.3)
    eng = _engine(m, rows_form="streamed")
    wd, wc = dev(m.ws, eng, torch.int32), _csr(m.ws, eng)
    a = _step(eng, m, eps, wd)
    b = _step(eng, m, eps, wc)
    c = _step(eng, m, eps, wd)
    d = _step(eng, m, eps, wc)
    _equal(a, b, torch.float64)
    assert a[0] == c[0] and b[0] == d[0]
    for name in a[2]:
        assert np.array_equal(a[2][name], c[2][name]) and np.array_equal(b[2][name], d[2][name]), name


def test_c_abi_rejects_mismatched_calls():
    from gdrf_amd import _lib
    m, eps = _loud_oracle(4, 30, 6, 5, torch.float64)
    eng = _engine(m, rows_form="auto")
    wd, wc = dev(m.ws, eng, torch.int32), _csr(m.ws, eng)
    assert eng._counts_ptr(wc) is None
    out = torch.empty(1, dtype=torch.float64, device=eng.device)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.GdrfHipError, match="ws_dev must be NULL"):
        _lib.check(eng.lib.gdrf_ll_const_dev(eng.ctx, wd.data_ptr(), m.N, out.data_ptr(), s), "gdrf_ll_const_dev")
    with pytest.raises(_lib.GdrfHipError, match="row count"):
        _lib.check(eng.lib.gdrf_ll_const_dev(eng.ctx, None, m.N - 1, out.data_ptr(), s), "gdrf_ll_const_dev")
    eng._counts_ptr(wd)
    _lib.check(eng.lib.gdrf_ll_const_dev(eng.ctx, wd.data_ptr(), m.N, out.data_ptr(), s), "gdrf_ll_const_dev")


# ---- 6. determinism
def test_sparse_is_bit_reproducible():
    m, eps = _loud_oracle(20, 300, 37, 9, torch.float32)
    _thin(m, 0.1)
    eng = _engine(m, rows_form="auto")
    ws = _csr(m.ws, eng)
    a = _step(eng, m, eps, ws)
    b = _step(eng, m, eps, ws)
    eng2 = _engine(m, rows_form="auto")
    c = _step(eng2, m, eps, _csr(m.ws, eng2))
    assert a[0] == b[0] == c[0]
    for name in a[2]:
        assert torch.equal(torch.from_numpy(a[2][name]), torch.from_numpy(b[2][name])), name
        assert torch.equal(torch.from_numpy(a[2][name]), torch.from_numpy(c[2][name])), name


# ---- 7. the model surface: five Adam steps follow the dense trajectory
def _model(xs, ws, V, K=3, dtype=torch.float64, **kw):
    from gdrf_amd import poutine
    from gdrf_amd.infer import SVI, Trace_ELBO
    from gdrf_amd.kernels import RBF
    from gdrf_amd.models import SparseMultinomialGDRF
    from gdrf_amd.optim import Adam
    model = SparseMultinomialGDRF(xs=xs, ws=ws, world=[(0.0, 1.0)] * 2,
                                  kernel=RBF(input_dim=2, lengthscale=torch.tensor(0.2), variance=torch.tensor(25.0)),
                                  num_observation_categories=V, num_topic_categories=K, dirichlet_param=0.01, n_points=[4, 3],
                                  fixed_inducing_points=True, inducing_init="grid", maxjitter=15, jitter=1e-6, device="cuda:0",
                                  dtype=dtype, seed=3, **kw)
    sc = poutine.scale(scale=1.0 / xs.shape[0])
    svi = SVI(model=sc(model.model), guide=sc(model.guide), optim=Adam({"lr": 1e-2}), loss=Trace_ELBO(num_particles=1))
    return model, svi


def _thin_counts(W, H, V, K, density, seed=8):
    from gdrf_amd.data import synth_circles
    xs_np, ws_np, _ = synth_circles(W, H, V, K, seed=seed)
    ws_np[np.random.default_rng(seed).random(ws_np.shape) > density] = 0
    return xs_np, ws_np


def test_sparse_five_adam_steps_through_svi_follow_the_dense_trajectory():
    from gdrf_amd.data import to_csr
    V = 400
    xs_np, ws_np = _thin_counts(14, 10, V, 3, 0.1)
    xs = torch.from_numpy(xs_np).to("cuda:0", torch.float64)
    wd = torch.from_numpy(ws_np).to("cuda:0")

    def run(ws, rows_form):
        model, svi = _model(xs, ws, V, rows_form=rows_form)
        g = torch.Generator().manual_seed(31)
        losses = [svi.step(xs=xs, ws=ws, subsample=False, eps=torch.randn(3, xs.shape[0], generator=g, dtype=torch.float64)) for _ in range(5)]
        ev = svi.evaluate_loss(xs=xs, ws=ws, eps=torch.randn(3, xs.shape[0], generator=g, dtype=torch.float64))
        return losses + [ev, float(model.perplexity(xs, ws))], model.state_dict()
    la, sa = run(wd, "streamed")
    lb, sb = run(to_csr(wd), "auto")
    assert np.allclose(lb, la, rtol=1e-8, atol=0), (la, lb)
    for k in sa:
        assert relerr(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 1e-8, k


# ---- 8. payload linearity over a row split cut with csr_rows
def _payload(eng, xs, ws, eps, n):
    lay = eng.red_layout
    eng.loss_and_grads(xs, ws, eps, n_global=n, force_level=0)
    torch.cuda.synchronize()
    return eng.red_T[:lay["total_T"]].double().cpu().numpy().copy(), eng.red_d[:4].cpu().numpy().copy()


def test_sparse_payload_is_linear_over_a_row_split():
    from gdrf_amd.data import csr_rows
    m, eps = _loud_oracle(10, 200, 37, 9, torch.float64)
    _thin(m, 0.1)
    eng = _engine(m, rows_form="auto")
    xs, e, ws = dev(m.xs, eng), dev(eps, eng), _csr(m.ws, eng)
    n, h = m.N, 150
    full = _payload(eng, xs, ws, e, n)
    a = _payload(eng, xs[:h], csr_rows(ws, slice(0, h)), e[:, :h].contiguous(), n)
    b = _payload(eng, xs[h:], csr_rows(ws, np.arange(h, n)), e[:, h:].contiguous(), n)
    lay = eng.red_layout
    assert relerr((a[0] + b[0])[:lay["GT"]], full[0][:lay["GT"]]) < 1e-10
    assert relerr(a[1] + b[1], full[1]) < 1e-12


# ---- 9. against the fp64 oracle where the LDS forms cannot run
def test_sparse_large_vocabulary_against_the_oracle():
    K, V, dtype = 5, 20_000, torch.float64
    m, eps = make_oracle(dtype=dtype, jitter=1e-6, W=37, H=9, V=V, K=K, n_points=(3, 2))
    rng = np.random.default_rng(4)
    ws = np.zeros((m.N, V), dtype=np.int32)
    for r in range(m.N):
        ws[r, rng.choice(V, size=20, replace=False)] = rng.integers(1, 30, size=20)
    m.ws = torch.from_numpy(ws)
    eng = _engine(m, rows_form="auto")
    loss, _, grads = _step(eng, m, eps, _csr(m.ws, eng))
    _vs_oracle(m, eps, eng, loss, grads)


def test_sparse_shape_whose_dense_counts_cannot_exist():
    """N = 70 000, V = 131 072: n x V = 9.2e9 count elements (37 GB as int32), 20 entries per row, built directly as CSR.  At
    initialisation Phi is uniform, so every p_v = 1 / V: perplexity = V and sum w log p = -(sum w) log V.  The second half of the rows
    sits past 2^32 dense elements; the payload is linear over the split."""
    from gdrf_amd.data import csr_rows
    N, V, K, per = 70_000, 131_072, 5, 20
    assert N * V > 2 ** 33
    g = torch.Generator(device="cuda:0").manual_seed(3)
    xs = torch.rand(N, 2, generator=g, device="cuda:0", dtype=torch.float64)
    col = torch.randint(0, V // per, (N, per), generator=g, device="cuda:0") + torch.arange(per, device="cuda:0") * (V // per)   # distinct inside a row
    val = torch.randint(1, 50, (N, per), generator=g, device="cuda:0", dtype=torch.int32)
    val[-64:] *= 1000                               # the last rows are loud
    ws = torch.sparse_csr_tensor(torch.arange(0, N * per + 1, per, device="cuda:0"), col.reshape(-1), val.reshape(-1), size=(N, V))
    model, _ = _model(xs, ws, V, K=K)
    tot = float(val.double().sum())
    eng = model._engine_for(N)
    s = eng.predict(xs, 3, ws).cpu().numpy()
    bound = 2.3e-16 * N * per
    assert s[1] == tot
    assert abs(s[0] + tot * math.log(V)) <= bound * tot * math.log(V), (s, tot)
    assert abs(float(model.perplexity(xs, ws)) - V) <= bound * V
    gc_ = torch.Generator().manual_seed(5)
    with torch.no_grad():
        eng.view("u_loc").add_(0.3 * torch.randn(eng.K, eng.M, generator=gc_, dtype=torch.float64).to(eng.device))
        eng.view("phi_unc").add_(0.5 * torch.randn(eng.K, V, generator=gc_, dtype=torch.float64).to(eng.device))
    eps = torch.randn(K, N, generator=g, device="cuda:0", dtype=torch.float64)
    h = N // 2
    full = _payload(eng, xs, ws, eps, N)
    a = _payload(eng, xs[:h], csr_rows(ws, slice(0, h)), eps[:, :h].contiguous(), N)
    b = _payload(eng, xs[h:], csr_rows(ws, slice(h, N)), eps[:, h:].contiguous(), N)
    lay = eng.red_layout
    pa, pb, pf = (x[0][lay["phibar"]:lay["A"]] for x in (a, b, full))
    assert relerr(pa + pb, pf) < 1e-10
    assert relerr(a[1] + b[1], full[1]) < 1e-12
    assert np.abs(pb).max() > 10 * np.abs(pa).max()          # the loud rows dominate the half that holds them
    del model, eng, ws
    gc.collect()
    torch.cuda.empty_cache()


# ---- 10. train()
@pytest.mark.parametrize("streaming", ["", "uniform"])
def test_train_on_csr_counts_returns_the_dense_history(streaming):
    from gdrf_amd.data import to_csr
    from gdrf_amd.train import train
    xs_np, ws_np = _thin_counts(12, 9, 300, 3, 0.1, seed=2)
    kw = dict(xs=xs_np, dimensions=2, num_topics=3, num_inducing_points=[4, 3], inducing_initialization_method="grid", jitter=1e-6,
              dtype=torch.float64, optimizer_lr=1e-2, streaming_inference=streaming, streaming_size=8)
    if streaming:
        kw.update(streaming_batch_splits=4)
    else:
        kw.update(epochs=4)
    a = train(ws=ws_np, rows_form="streamed", **kw)["history"]
    b = train(ws=to_csr(ws_np), **kw)["history"]
    c = train(ws=ws_np, sparse=True, **kw)["history"]
    assert a.shape == b.shape and np.allclose(b, a, rtol=1e-8, atol=0), (a, b)
    assert np.array_equal(b, c)


# ---- 11. two ranks on one GPU, each with its CSR shard (the dense check: tests/test_gpu_surface.py)
def _build_csr(lo=None, hi=None):
    """tests/test_gpu_surface.py's fp64 model on thinned counts held as CSR; the SVI object and this rank's rows [lo, hi) of them"""
    from gdrf_amd.data import csr_rows, to_csr
    V, K = 60, 4
    xs_np, ws_np = _thin_counts(30, 20, V, K, 0.15, seed=3)
    xs = torch.from_numpy(xs_np).to("cuda:0", torch.float64)
    ws = to_csr(torch.from_numpy(ws_np).to("cuda:0"))
    model, svi = _model(xs, ws, V, K=K)
    if lo is None:
        return model, svi, xs, ws
    return model, svi, xs[lo:hi], csr_rows(ws, slice(lo, hi))


def _dist_worker_csr(rank, world, port, tmp):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)          # both ranks share the single GPU
    N = 30 * 20
    lo, hi = rank * N // world, (rank + 1) * N // world
    model, svi, xs, ws = _build_csr(lo, hi)
    assert ws.layout == torch.sparse_csr and ws.shape[0] == hi - lo
    svi.row_offset = lo
    if os.environ.get("GDRF_TEST_C_ABI_ALLREDUCE") == "1":               # the collective registered behind the C ABI
        eng = model._engine_for(hi - lo)
        eng.pg = None

        def allreduce(buf, count, is_double, stream):
            assert buf == eng.red_T.data_ptr() and count == eng.red_T.numel() and is_double
            dist.all_reduce(eng.red_T)
            return 0
        eng.set_allreduce(allreduce)
    losses = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(3)]
    assert model._engine._csr_bound
    torch.save({"losses": losses, "params": model._engine.params.cpu()}, os.path.join(tmp, f"r{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("via", ["torch_distributed", "c_abi_hook"])
def test_two_ranks_with_csr_shards_match_a_single_rank(tmp_path, via, monkeypatch):
    import os
    import torch.multiprocessing as mp
    monkeypatch.setenv("GDRF_TEST_C_ABI_ALLREDUCE", "1" if via == "c_abi_hook" else "0")
    port = 33600 + (os.getpid() % 2000) + (7 if via == "c_abi_hook" else 0)
    mp.spawn(_dist_worker_csr, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    model, svi, xs, ws = _build_csr()
    ref = [svi.step(xs=xs, ws=ws, subsample=False) for _ in range(3)]
    r0 = torch.load(tmp_path / "r0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert r0["losses"] == r1["losses"]
    assert np.allclose(r0["losses"], ref, rtol=1e-10)                      # Philox keyed by the global row: same eps
    assert torch.equal(r0["params"], r1["params"])
    assert (r0["params"] - model._engine.params.cpu()).abs().max() < 1e-9
