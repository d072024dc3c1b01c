"""CPU side of the sweep over the two side paths of a training step: the custom-link step (gdrf_step_local_link) and the two-point step of a
non-unit world (gdrf_step_local2).  Case tables, builders and references, held once: tests/test_gpu_side_edges.py steps the engine on them,
tests/test_side_edges_host.py shows from the reference alone that they cross the edges they name.  Imports oracle/ and the test helpers, never
the engine.

A case is a dict (``case()`` lists the keys).  ``build(c)`` returns (oracle, eps, xs_world): a float64 RefShapedGDRF on a W x H lattice whose
data are loud in the sense of tests/test_gpu_rows.py::_loud_oracle - the last row has ~100 x the counts of the others, word V - 1 the largest
counts, topic K - 1 the largest u_loc, ``zero_rows`` rows have no counts - with a contracted guide (trained_scale), so that |mu| stays O(10).
float32 cases follow the project's protocol: parameters, Z, eps and the inputs are float32 VALUES in the float64 oracle.

``row_reference`` is the per-row reference: autograd through the oracle's own formulas with respect to the predictive's (loc, var) at the
model's and the guide's inputs.  Nothing of the kernels' hand-derived adjoints is restated."""
import math

import numpy as np
import torch
from torch.distributions import Dirichlet, Multinomial, Normal

from oracle.gdrf_oracle import RefShapedGDRF, conditional, kernel_matrix
from tests._util import perturb_posterior
from tests.test_gpu_round2 import _LINKS, WORLD
from tests.test_gpu_round3 import _fp32_valued
from tests.test_gpu_sparse import _thin
from tests.test_gpu_vocab_stream import _clamp_word

JITTER = {"fp64": 1e-6, "fp32": 1e-4}
# Where the true value is 0 (V = 1, or every word clamped: no likelihood gradient, and the two Normal sites cancel in d / d f_loc) autograd
# answers with float64 round-off of the cancelling O(1) terms, measured 7e-18; differences below this floor are not errors of either side
ABS_FLOOR = 1e-14
SEED = 3
MEAN_FN = lambda x: 1.5 * x[:, 0] - 0.7 * x[:, 1]                      # noqa: E731
PRODUCT = [("kern0", "rbf", [0], 0.6, 2.0, None), ("kern1", "periodic", [1], 0.8, 1.5, 0.45)]      # RBF(axis 0) x Periodic(axis 1)

# ---- constants of csrc/rows_vstream.h, csrc/api.hip and csrc/forms.h, restated once (test_side_edges_host.py ties each to its source line)
RB = 64                                   # VsCfg<T>::RB: rows of a block of the streamed kernel, and of a workgroup pass of the V-free kernels
VT = {8: 32, 4: 64}                       # VsCfg<T>::VT by element size: words of a Phi tile
KJ_SPLIT = 32                             # rows_vstream_kernel<T, MODE, 8> up to this K, <.., 32> above
GCAP_BYTES = 256 << 20                    # vs_ensure: the Phi-bar partial slots stay under this many bytes (but at least 16 slots)
GRID_MAX = 1024
F_TILE = 128
W1_PAIRS = 32                             # w1_gate: row-tile pairs x column tiles above this


def sparse_form(K):
    """(LG, KJ) of rows_csr_kernel (api.hip: sparse_form)"""
    return (8, 1) if K <= 8 else (16, 2) if K <= 32 else (16, 8)


def derived(c):
    """What the launch derives from a case's shape."""
    W, H = c["lattice"]
    n, esz = W * H, 8 if c["regime"] == "fp64" else 4
    n_cap = c["n_cap"] or n
    K, V = c["K"], c["V"]
    M = int(np.prod(c["n_points"]))
    Mp = (M + 31) // 32 * 32
    nblk = (n + RB - 1) // RB
    gcap = min(GRID_MAX, max(16, GCAP_BYTES // (K * V * esz)), (n_cap + RB - 1) // RB)
    grid = max(1, min(nblk, GRID_MAX if c["route"] == "csr" else gcap))
    rtiles = (n + F_TILE - 1) // F_TILE
    pairs, nt = (rtiles + 1) // 2, (Mp + F_TILE - 1) // F_TILE
    nkb = Mp // 64
    return dict(n=n, ldk=(n_cap + 3) // 4 * 4, row_blocks=nblk, ragged=n % RB, grid=grid, blocks_per_wg=-(-nblk // grid), KJ=8 if K <= KJ_SPLIT else 32,
                LG=sparse_form(K)[0], csr_KJ=sparse_form(K)[1], vt_tiles=-(-V // VT[esz]), vt_ragged=V % VT[esz], Mp=Mp, pairs=pairs, nt=nt,
                w1=Mp % 64 == 0 and 2 <= K <= 16 and pairs * nt > W1_PAIRS, nslice=min(nkb, 8) if (pairs * nt <= W1_PAIRS and nkb >= 2) else 1)


# ---- the case tables --------------------------------------------------------------------------------------------------------------------
def case(id, path, K, V, **kw):
    c = dict(id=id, path=path, K=K, V=V, lattice=(37, 9), n_points=(4, 3), kind="rbf", regime="fp64", whiten=True, learn=False, mean=False,
             clamp_word=None, zero_rows=3, link=None, route="dense", density=1.0, n_cap=None, particles=1, renyi=None, mfma_mode="auto",
             store_t="auto", hyper_backward="auto", product=False, forms=None)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return c


LINK_EDGES = [(1, 1), (1, 2), (8, 31), (9, 32), (32, 33), (33, 63), (33, 64), (33, 65), (128, 33), (128, 65)]
LINK_CLAMP = [(1, 2), (9, 32), (33, 65), (128, 33)]
CAPPED = dict(K=128, V=4100, lattice=(67, 61))           # tests/test_gpu_vocab_stream.py::test_streamed_more_row_blocks_than_the_capped_grid
CSR_BIG = dict(K=3, V=9, lattice=(2851, 23))             # 1024 x 64 + 37 rows: every workgroup of the 1024-wide grid takes a second block
TWO_EDGES = [(1, 2), (9, 32), (32, 64), (33, 65), (128, 33)]
W1_LATTICE = (97, 89)                                    # 8633 rows: 34 row-tile pairs


def _link_cases():
    out = []
    for regime in ("fp64", "fp32"):
        for K, V in LINK_EDGES:
            for link in ("sigmoid", "tempered_softmax"):
                out.append(case(f"link-{link}-K{K}-V{V}-{regime}", "link", K, V, link=link, regime=regime))
    for K, V in LINK_CLAMP:
        out.append(case(f"link-clamp-K{K}-V{V}-fp64", "link", K, V, link="sigmoid", clamp_word=V // 2))
    out.append(case("link-clamp-K9-V32-fp32", "link", 9, 32, link="sigmoid", clamp_word=16, regime="fp32"))
    out.append(case("link-ncap401-K9-V32", "link", 9, 32, link="sigmoid", n_cap=401))
    out.append(case("link-capped-grid-K128-V4100", "link", link="sigmoid", **CAPPED))
    out.append(case("link-particles3-K9-V32", "link", 9, 32, link="sigmoid", particles=3))
    out.append(case("link-renyi-K9-V32", "link", 9, 32, link="sigmoid", particles=3, renyi=0.5))
    for K in (8, 9, 32, 33, 128):
        for density in (0.05, 1.0):
            out.append(case(f"link-csr-K{K}-V50-d{density}", "link", K, 50, link="sigmoid", route="csr", density=density))
    out.append(case("link-csr-clamp-K9-V50", "link", 9, 50, link="sigmoid", route="csr", density=0.3, clamp_word=25))
    for K in (9, 33):
        out.append(case(f"link-csr-K{K}-V50-fp32", "link", K, 50, link="sigmoid", route="csr", density=0.3, regime="fp32"))
    out.append(case("link-csr-two-blocks-per-workgroup", "link", link="sigmoid", route="csr", density=0.3, **CSR_BIG))
    return out


def _two_cases():
    out = []
    for regime in ("fp64", "fp32"):
        for K, V in TWO_EDGES:
            out.append(case(f"two-K{K}-V{V}-{regime}", "two", K, V, regime=regime, mfma_mode="auto" if regime == "fp64" else "f16x3"))
    for K in (9, 33):
        out.append(case(f"two-csr-K{K}-V50", "two", K, 50, route="csr", density=0.3))
    opt = lambda name, **kw: out.append(case("two-" + name, "two", 4, 20, **kw))      # noqa: E731
    opt("learn-inducing", learn=True)
    for kind in ("matern52", "matern32", "exponential", "rationalquadratic"):
        opt(kind, kind=kind)
    opt("unwhitened-learn-inducing", whiten=False, learn=True)
    opt("product-rbf0-periodic1", product=True)
    opt("mean", mean=True)
    opt("particles3", particles=3)
    opt("renyi", particles=3, renyi=0.5)
    opt("ncap401", n_cap=401)
    for mode in ("f16x3", "bf16x6", "f32"):
        opt("fp32-" + mode, regime="fp32", mfma_mode=mode)
    opt("fp32-hyper-tn", regime="fp32", mfma_mode="f16x3", hyper_backward="tn")
    # the forms of W-bar and tt that read bwd_vscale's scaled copies of vbar and asum, which the guide-side backward must find swapped too
    opt("fp32-w1-forms", regime="fp32", mfma_mode="f16x3", n_points=(8, 8), lattice=W1_LATTICE, forms=dict(wbar="w1", wbar_nslice=1, fwd_t="w1"))
    opt("fp32-k64-form", regime="fp32", mfma_mode="f16x3", n_points=(8, 8), forms=dict(wbar="k64", wbar_nslice=1))
    opt("fp32-k64-sliced", regime="fp32", mfma_mode="f16x3", n_points=(16, 8), forms=dict(wbar="k64", wbar_nslice=2))    # Mp = 128: two reduction slices
    return out


LINK_CASES = _link_cases()
TWO_CASES = _two_cases()
CASES = {c["id"]: c for c in LINK_CASES + TWO_CASES}
assert len(CASES) == len(LINK_CASES) + len(TWO_CASES)
LARGE = ("link-capped-grid-K128-V4100", "link-csr-two-blocks-per-workgroup", "two-fp32-w1-forms")      # the three that take seconds


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def _lattice(W, H):
    gx, gy = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    idx = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64)
    return torch.from_numpy(idx / idx.max(0, keepdims=True))


def _loud_counts(N, V, zero_rows, clamp_word, rng):
    ws = rng.integers(0, 8, size=(N, V))
    ws[:, V - 1] += rng.integers(20, 60, size=N)
    ws[N - 1] *= 100
    if clamp_word is not None:
        ws[:, clamp_word] = 3
    if zero_rows:
        ws[rng.choice(N - 1, size=zero_rows, replace=False)] = 0
    return ws.astype(np.int32)


def build(c):
    """(oracle, eps, xs_world) of a case.  eps is (K, N), or (P, K, N) with particles; xs_world are the observations in world coordinates
    (two-point cases; the unit-cube inputs themselves on the link path)."""
    K, V, (W, H) = c["K"], c["V"], c["lattice"]
    two, fp32 = c["path"] == "two", c["regime"] == "fp32"
    g = torch.Generator().manual_seed(SEED + 100)
    rng = np.random.default_rng(SEED)
    xs = _lattice(W, H)
    if fp32:
        xs = xs.float().double()
    if two:
        lower = torch.tensor([w[0] for w in WORLD], dtype=torch.float64)
        delta = torch.tensor([w[1] - w[0] for w in WORLD], dtype=torch.float64)
        xs = xs * delta + lower
    M = int(np.prod(c["n_points"]))
    Z = (0.05 + 0.9 * torch.rand(M, 2, generator=g, dtype=torch.float64)) if c["learn"] else None      # interior: no vanishing sigmoid Jacobian
    ws = _loud_counts(W * H, V, c["zero_rows"], c["clamp_word"], rng)
    kw = dict(kind="rbf", lengthscale=0.5, variance=1.0) if c["product"] else dict(kind=c["kind"], lengthscale=0.3)
    m = RefShapedGDRF(xs, ws, K=K, n_points=c["n_points"], dtype=torch.float64, jitter=JITTER[c["regime"]], Z=Z, learn_inducing=c["learn"],
                      whiten=c["whiten"], mean_function=MEAN_FN if c["mean"] else None, world=WORLD if two else None, guide_rescale=True,
                      link_function=_LINKS[c["link"]] if c["link"] else None, optimizer="adam", lr=1e-2, **kw)
    if c["product"]:
        m.set_factors(PRODUCT)
    perturb_posterior(m, g, trained_scale=0.1)
    if c["density"] < 1.0:
        _thin(m, c["density"])
        if c["clamp_word"] is not None:                    # the clamp sits at a STORED entry of every row with counts
            with torch.no_grad():
                w = m.ws.clone()
                w[w.sum(1) > 0, c["clamp_word"]] = 3
                m.ws = w
    # f_k = K_nm K_uu^-1 u_k (whitened: W u_k with W L^T = K_nm): lifting u_{K-1} by L^T c (K_uu c) lifts f_{K-1} by K_nm c > 0 everywhere
    with torch.no_grad():
        L = m._luu(m.constrained())
        lift = torch.full((M,), 0.2, dtype=torch.float64)
        m.params["u_loc"][K - 1] += (L.T @ lift) if c["whiten"] else (L @ (L.T @ lift))
    if c["clamp_word"] is not None:
        _clamp_word(m, c["clamp_word"])
    P = c["particles"]
    eps = torch.randn(*((P,) if P > 1 else ()), K, m.N, generator=g, dtype=torch.float64)
    if fp32:
        _fp32_valued(m)
        eps = eps.float().double()
    return m, eps, xs


def oracle_loss_and_grads(m, c, eps, level=None):
    """RefShapedGDRF.loss_and_grads of the case's estimator at jitter level ``level`` (None: the oracle's own): Trace_ELBO's mean over the
    particles, or RenyiELBO."""
    m.force_jitter_level = level
    if c["renyi"] is not None:
        return m.loss_and_grads(eps, renyi_alpha=c["renyi"])
    if eps.dim() == 2:
        return m.loss_and_grads(eps)
    res = [m.loss_and_grads(e) for e in eps]
    return float(np.mean([r[0] for r in res])), {k: sum(r[1][k] for r in res) / len(res) for k in res[0][1]}


def eps32_loss_shift(m, c):
    """What a float32 evaluation adds to the float64 loss in a clamp case: every count on the clamped word sees log(eps32) in place of
    log(eps64) (tests/test_gpu_round3.py::test_multinomial_eps_clamp_and_zero_count_branches)."""
    w = float(m.ws[:, c["clamp_word"]].sum())
    return -w * (math.log(np.finfo(np.float32).eps) - math.log(np.finfo(np.float64).eps)) / m.N


# ---- the row reference ------------------------------------------------------------------------------------------------------------------
def _predictive(m, c, Luu, x):
    Z = m.inducing()
    loc, var = conditional(m.kind, x, Z, c["lengthscale"], c["variance"], c["u_loc"], c["u_scale_tril"], Luu, c["scale_mixture"], m.whiten,
                           **c["kernel_kw"])
    if m.mean_function is not None:
        loc = loc + m.mean_function(x)
    Kfs = kernel_matrix(m.kind, Z, x, c["lengthscale"], c["variance"], c["scale_mixture"], **c["kernel_kw"])
    W = torch.linalg.solve_triangular(Luu, Kfs, upper=False).t()              # the conditional's own W: its Qss diagonal is sum_j W_nj^2
    return loc, var, W


def row_reference(m, eps, level=None, normaliser="unclamped"):
    """Per-row values and adjoints of one evaluation (one particle: eps is (K, N)), float64 torch.

    Leaves: (f_loc_m, f_var_m) and (f_loc_g, f_var_g), the oracle's ``conditional`` at the model's and the guide's inputs; one pair on the
    single-point (link) path.  mu and the unscaled row terms lp_mu + ll - lq_mu are formed as RefShapedGDRF.loss forms them, and autograd
    gives locbar, vbar (model side; both sides together on the single-point path) and g_locbar, g_vbar (guide side).

    ``normaliser="all"`` is the fault a clamp case exists for: the likelihood's normaliser term -(sum of counts) log(sum p) taken over ALL
    counts of a row instead of the ones inside the clamp range (a `cn` that forgot the clamp)."""
    m.force_jitter_level = level
    two = m.world is not None and m.guide_rescale
    with torch.no_grad():
        c = m.constrained()
        Luu = m._luu(c)
        xs_m = m.scale(m.xs)
        loc_m, var_m, W_m = _predictive(m, c, Luu, xs_m)
        loc_g, var_g, W_g = _predictive(m, c, Luu, m.scale(xs_m)) if two else (loc_m, var_m, W_m)
        noise, phi = c["noise"], c["phi"]
    leaves = [t.clone().requires_grad_(True) for t in ((loc_m, var_m, loc_g, var_g) if two else (loc_m, var_m))]
    f_loc_m, f_var_m = leaves[0], leaves[1]
    f_loc_g, f_var_g = (leaves[2], leaves[3]) if two else (f_loc_m, f_var_m)
    mu = f_loc_g + f_var_g * eps
    lq_mu = Normal(f_loc_g, f_var_g).log_prob(mu).sum()
    lp_mu = Normal(f_loc_m, f_var_m + noise).log_prob(mu).sum()
    theta = m.link_function(mu)
    probs = torch.matmul(theta.transpose(-2, -1), phi)
    if normaliser == "unclamped":
        ll = Multinomial(probs=probs, validate_args=False).log_prob(m.ws).sum()
    else:
        fe = torch.finfo(torch.float64).eps
        w = m.ws.double()
        ph = (probs / probs.sum(-1, keepdim=True)).detach()
        inr = ((ph > fe) & (ph < 1 - fe)).double()
        ll = (w * inr * probs.log()).sum() - (w.sum(-1) * probs.sum(-1).log()).sum()
    total = lp_mu + ll - lq_mu
    grads = torch.autograd.grad(total, leaves)
    fe64 = torch.finfo(torch.float64).eps
    ph_ = (probs / probs.sum(-1, keepdim=True)).detach()
    cn = (m.ws.double() * ((ph_ > fe64) & (ph_ < 1 - fe64)).double()).sum(-1) / probs.detach().sum(-1)
    out = dict(cn=cn, q=W_m.pow(2).sum(-1), mu=mu.detach(), locbar=grads[0], vbar=grads[1], W_m=W_m, W_g=W_g, Luu=Luu, theta=theta.detach(),
               p_hat=(probs / probs.sum(-1, keepdim=True)).detach(), two=two)
    if two:
        out.update(g_locbar=grads[2], g_vbar=grads[3])
    return out


def link_cancellation_floor(m, ref, V, feps):
    """(K, N) absolute floor of the link path's row adjoint, from the precision of the element type (``feps`` its epsilon).

    The link kernels form the likelihood's pull-back to theta as thetabar_k - cn rowsum_k: a sum of V terms w_v phi_kv / p_v that adds up
    to about cn = (unclamped counts) / sum p, less that constant.  Each side carries a rounding error of up to (V + 2) feps cn (the
    standard bound for a V-term sum and the two products), whatever the size of the difference - which is exactly 0 for K = 1, where the
    normalised p does not depend on the one theta at all, and there autograd's own answer is float64 round-off around 0 too.  The caller's
    Jacobian then maps it to mu: |J^T e|_k <= sum_j |d theta_j / d mu_k| max|e|.  At the shapes with K > 1 the floor is far below the
    bounds (tests/test_side_edges_host.py checks that), so it loosens nothing there."""
    mu = ref["mu"].clone().requires_grad_(True)
    theta = m.link_function(mu)
    abs_j = torch.zeros_like(mu)
    for j in range(theta.shape[0]):
        (g,) = torch.autograd.grad(theta[j].sum(), mu, retain_graph=True)
        abs_j += g.abs()
    return (V + 2) * feps * ref["cn"][None, :] * abs_j


def u_loc_grad_from_rows(m, ref):
    """d loss / d u_loc from the row adjoints: -1/N (locbar W_m + g_locbar W_g), through L^-1 in an unwhitened context (f_loc = W L^-1 u)."""
    g = ref["locbar"] @ ref["W_m"]
    if ref["two"]:
        g = g + ref["g_locbar"] @ ref["W_g"]
    if not m.whiten:
        g = torch.linalg.solve_triangular(ref["Luu"].T, g.T, upper=True).T
    return -g / m.N


def dirichlet_grad(m):
    """d loss / d phi_unc of the Dirichlet prior term alone"""
    p = m.params["phi_unc"].detach().clone().requires_grad_(True)
    lp = Dirichlet(m.alpha).log_prob(torch.softmax(p, -1)).sum()
    return -torch.autograd.grad(lp, p)[0] / m.N
