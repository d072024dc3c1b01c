"""A plain numpy restatement of the predictive mean path (gdrf_predict modes 0-4, include/gdrf_hip.h), the shapes at which
tests/test_gpu_predict_forms.py runs it and the error bound of each.  CPU only: it imports neither the engine nor the oracle.

The operation, straight from the definitions:  K_uu + jitter I  ->  its Cholesky factor L (a column loop, so that it runs in any numpy
dtype)  ->  L^-1 by forward substitution  ->  Cf = L^-T u  (whiten = False: u <- L^-1 u first)  ->  loc = K_nm Cf  ->  theta = softmax
over the topics  ->  Phi = softmax(phi_unc)  ->  p = theta Phi  ->  {sum w log p, sum w};  mode 4 adds
var = clamp(variance - |w|^2, 0) + |S_k^T w|^2 with w = L^-1 k(Z, x).

It is evaluated twice per group of cases:
  exact        everything in np.longdouble (64-bit significand; the module that imports this one is skipped where numpy has none);
  as designed  the same route in the arithmetic the design prescribes for the context type: the solve precision (float64 for GDRF_F64
               and GDRF_F32, float32 for GDRF_F32_PURE) for K_uu, L, L^-1, Cf, the covariance values, loc and the softmax, the array
               precision for Phi and the stored outputs (and, in mode 4, for the contractions over the stored W).
The bound of a case comes from these two alone, never from the device:  e_ref = relerr(as designed, exact) per mode, and a case passes
when relerr(device, exact) <= 64 e_ref + floor, floor = 1e-13 for float64 outputs and 2^-23 for float32 outputs.  The factor 64: the
device adds the M terms in another order (four per matrix instruction) and evaluates 2^t by a polynomial whose argument rounding is of
the order of the library's; the floor covers a restatement that happens to round luckily.  CEILING (the suite's 1e-9 / 5e-4) is what the
computed bound may never exceed (tests/test_predict_forms_host.py asserts it for every shape below).

Inputs: grid inducing points, lengthscale = 1.5 x the grid spacing (per axis for ARD, the widest axis otherwise), variance 25, jitter
1e-6 (1e-4 in the float32 context types, where every input is a float32 value).
"""
import functools

import numpy as np

LD = np.longdouble
HAS_LONGDOUBLE = bool(np.finfo(LD).eps < 1e-18)
KINDS = ("rbf", "matern52", "matern32", "exponential", "rationalquadratic")
CTX = {  # context type -> (solve precision, array precision, jitter)
    "f64": (np.float64, np.float64, 1e-6),
    "f32": (np.float64, np.float32, 1e-4),
    "pure": (np.float32, np.float32, 1e-4),
}
CEILING = {"f64": 1e-9, "f32": 5e-4, "pure": 5e-4}
FACTOR = 64.0
FLOOR = {np.dtype(np.float64): 1e-13, np.dtype(np.float32): 2.0 ** -23}
DMAX, KMAX = 4, 32                     # GDRF_DMAX, GDRF_KMAX of csrc/common.h
LDS_FORM, LDS_MAX = 64 * 1024, 150 * 1024
GRID_ROWS_MFMA, GRID_ROWS = 2048 * 4 * 16, 2048 * 128      # rows one pass of the capped grids covers


def relerr(a, b):
    """max |a - b| / max |b|, formed in long double (a float64 difference of two results 1e-16 apart would be all rounding)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / (np.abs(b).max() + LD(1e-300)))


def measure(got, exact):
    """The tests' measure of an output: relerr, and infinity if any element is not finite (a NaN sentinel left in place)."""
    got = np.asarray(got)
    return relerr(got, exact) if np.isfinite(got.astype(np.float64)).all() else float("inf")


# ---- the dispatch of predict() (csrc/api.hip), restated for choosing shapes ---------------------------------------------------------------

def lds_bytes(form, M, D, K, V, ts):
    """Dynamic LDS of a predictive form, ts = the size of a solve-precision element."""
    if form == 1:
        M4, DD, NB = (M + 3) // 4 * 4, (2 if D <= 2 else DMAX), (1 if K <= 16 else 2)
        return 128 + (M4 * DD + K * V + 4 * 16 * (16 * NB + 1)) * ts
    if form == 2:
        return 128 + (M * D + K * V + K * M) * ts
    if form == 3:
        return 128 + (M * D + K * V) * ts
    return 128 + (M * D + K * V + 128 * (V + 1)) * ts


def expected_form(M, D, K, V, ts, streamed=False):
    """(GDRF_FORM_PREDICT, GDRF_FORM_PREDICT_NB) predict() picks for modes 0-3."""
    if streamed:
        return 5, 0
    if K <= KMAX and lds_bytes(1, M, D, K, V, ts) <= LDS_FORM:
        return 1, (1 if K <= 16 else 2)
    if K > KMAX:
        return 4, 0
    return (2, 0) if lds_bytes(2, M, D, K, V, ts) <= LDS_FORM else (3, 0)


def vocab_for(form, M, D, K, ts):
    """The smallest V at which a K <= 32 shape leaves the matrix-core form for `form` (2 or 3)."""
    for V in range(1, 1 << 16):
        if expected_form(M, D, K, V, ts)[0] == form:
            assert lds_bytes(3, M, D, K, V, ts) <= LDS_MAX
            return V
    raise AssertionError("no such V")


# ---- the restatement --------------------------------------------------------------------------------------------------------------------

def cholesky(A):
    """Lower Cholesky factor by a column loop, in A's dtype."""
    M = A.shape[0]
    L = np.zeros_like(A)
    for j in range(M):
        d = A[j, j] - np.sum(L[j, :j] * L[j, :j], dtype=A.dtype)
        assert d > 0, "K_uu + jitter I is not positive definite in this arithmetic"
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, M):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j], dtype=A.dtype)) / L[j, j]
    return L


def lower_inverse(L):
    """L^-1 by forward substitution, row by row, in L's dtype."""
    M = L.shape[0]
    X = np.zeros_like(L)
    eye = np.eye(M, dtype=L.dtype)
    for i in range(M):
        X[i] = (eye[i] - (L[i, :i, None] * X[:i]).sum(0, dtype=L.dtype)) / L[i, i]
    return X


def covariance(kind, X, Z, ls, var, alpha, t):
    """k(x_n, z_i) in dtype t from the direct (x - z)^2 form, pyro's isotropic kernels (Matern and Exponential take r = sqrt(r2 + 1e-12))."""
    sx, sz = X.astype(t) / ls.astype(t), Z.astype(t) / ls.astype(t)
    r2 = np.zeros((X.shape[0], Z.shape[0]), dtype=t)
    for d in range(X.shape[1]):
        df = sx[:, d, None] - sz[None, :, d]
        r2 += df * df
    var, alpha = t(var), t(alpha)
    if kind == "rbf":
        return var * np.exp(t(-0.5) * r2)
    if kind == "rationalquadratic":
        return var * np.exp(-alpha * np.log(t(1) + r2 * (t(0.5) / alpha)))
    r = np.sqrt(r2 + t(1e-12))
    if kind == "exponential":
        return var * np.exp(-r)
    if kind == "matern32":
        a = np.sqrt(t(3)) * r
        return var * (t(1) + a) * np.exp(-a)
    a = np.sqrt(t(5)) * r
    return var * (t(1) + a + (t(5) / t(3)) * r * r) * np.exp(-a)


def softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True, dtype=x.dtype)


def restate(inp, kind, solve, array, whiten=True, with_var=False, need_p=True):
    """loc (K, n), theta (n, K), p (n, V) [and var (K, n)] of the inputs `inp` in the given solve and array precisions; the stored
    outputs are rounded to `array`.  The hyper-parameters are the exponentials of the stored (array-valued) unconstrained ones, taken in
    double by the library and in `solve` here when that is wider."""
    hp = solve if np.finfo(solve).bits >= 64 else np.float64
    ls = np.exp(np.atleast_1d(inp["log_ls"]).astype(hp)) * np.ones(inp["X"].shape[1], dtype=hp)
    var, alpha = np.exp(hp(inp["log_var"])), np.exp(hp(inp["log_alpha"]))
    Z, X = inp["Z"], inp["X"]
    Kuu = covariance(kind, Z, Z, ls, var, alpha, solve) + solve(inp["jitter"]) * np.eye(Z.shape[0], dtype=solve)
    Linv = lower_inverse(cholesky(Kuu))
    u = inp["u"].astype(solve)                                         # (K, M)
    if not whiten:
        u = (Linv[None] * u[:, None, :]).sum(-1, dtype=solve)          # L^-1 u_k
    Knm = covariance(kind, X, Z, ls, var, alpha, solve)                # (n, M)
    out = {}
    if with_var:
        # mode 4: the step's forward.  W = K_nm L^-T in the solve precision, stored in the array precision; the contractions over it
        # (loc = W U^T, |w|^2, |S_k^T w|^2) run in the array precision
        W = (Knm @ Linv.T).astype(array) if solve is not LD else Knm @ Linv.T
        a = array if solve is not LD else LD
        S = np.tril(inp["S_unc"], -1) + np.exp(np.diagonal(inp["S_unc"], axis1=1, axis2=2).astype(hp))[:, :, None] * np.eye(Z.shape[0])
        S = S.astype(solve)
        if not whiten:
            S = np.einsum("ij,kjl->kil", Linv, S)
        S = S.astype(a)
        out["loc4"] = (W @ u.astype(a).T).T.astype(a)
        q = (W * W).sum(1, dtype=a)
        tt = np.stack([((W @ S[k]) ** 2).sum(1, dtype=a) for k in range(S.shape[0])])
        out["var"] = (np.maximum(a(var) - q, a(0))[None] + tt).astype(a)
        return out
    Cf = (Linv.T[None] * u[:, None, :]).sum(-1, dtype=solve)           # (K, M): L^-T u_k
    loc = (Knm @ Cf.T).T                                               # (K, n)
    out["Knm"], out["Cf"] = Knm, Cf
    theta = softmax(loc, 0).T                                          # (n, K)
    arr = array if solve is not LD else LD
    out["loc"], out["theta"] = loc.astype(arr), theta.astype(arr)
    if not need_p:
        return out
    phi = softmax(inp["phi_unc"].astype(arr), 1).astype(solve)
    p = theta @ phi
    out["p"] = p.astype(arr)
    out["logp"] = np.log(p)                                            # solve precision: the perplexity sums never round p
    return out


def perp_sums(logp, ws):
    """{sum w log p, sum w} over the rows given, the first in long double and returned as such."""
    w = ws.astype(LD)
    return LD((w * logp.astype(LD)).sum()), int(ws.astype(np.int64).sum())


def perplexity(s0, s1):
    """exp(-sum w log p / sum w) in long double: the figure mode 3 is compared by.  Its relative error is |delta sum w log p| / sum w, which
    stays meaningful where sum w log p itself vanishes (V = 1: p = 1)."""
    return np.exp(-LD(s0) / LD(s1))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def grid_points(grid, D):
    """The unit-cube grid of `grid` points per axis (an axis with one point sits at 0.5), (M, D)."""
    axes = [np.linspace(0.0, 1.0, g) if g > 1 else np.array([0.5]) for g in grid] + [np.array([0.5])] * (D - len(grid))
    return np.stack([a.flatten() for a in np.meshgrid(*axes, indexing="ij")], -1).reshape(-1, D)


def make_inputs(g):
    """The inputs of a group at its largest n; smaller n take the leading rows.  float32-valued in the float32 context types."""
    rng = np.random.default_rng(g.get("seed", 7))
    D, K, V, grid = g["D"], g["K"], g["V"], g["grid"]
    nmax = max(g["ns"])
    Z = grid_points(grid, D)
    M = Z.shape[0]
    spacing = np.array([1.0 / (gd - 1) if gd > 1 else 0.0 for gd in grid] + [0.0] * (D - len(grid)))
    wide = spacing.max()
    if g.get("ard"):           # unequal lengthscales: 1.5 x each axis' own spacing, an axis with one point 1.5 x the widest, then spread
        ls = 1.5 * np.where(spacing > 0, spacing, wide) * (1.0 + 0.15 * np.arange(D))
    else:
        ls = np.array(1.5 * wide)
    inp = dict(X=rng.random((nmax, D)), Z=Z, log_ls=np.log(ls), log_var=np.log(25.0), log_alpha=np.log(g.get("alpha", 1.0)),
               u=0.3 * rng.standard_normal((K, M)), phi_unc=0.5 * rng.standard_normal((K, V)),
               ws=rng.integers(0, 9, (nmax if 3 in g["modes"] else 1, V)).astype(np.int32), jitter=CTX[g["ctx"]][2])
    if g.get("mode4"):
        S = 0.1 * np.tril(rng.standard_normal((K, M, M)), -1)
        inp["S_unc"] = S + np.log(0.5) * np.eye(M)[None]
    if g["ctx"] != "f64":
        for k, v in inp.items():
            if k not in ("ws", "jitter"):
                inp[k] = np.asarray(v, dtype=np.float32).astype(np.float64)
    return inp


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def _g(id, **kw):
    g = dict(id=id, ctx="f64", kind="rbf", D=2, ard=False, grid=(3, 3), K=5, V=7, ns=(37,), modes=(0, 1, 2, 3), whiten=True,
             streamed=False, n_cap=None, csr=False, mode4=False, n1=None)
    g.update(kw)
    g["M"] = int(np.prod(g["grid"]))
    ts = np.dtype(CTX[g["ctx"]][0]).itemsize
    if isinstance(g["V"], str):                    # "rows_lds" / "rows_mem": V from the LDS formulas of predict()
        g["V"] = vocab_for(2 if g["V"] == "rows_lds" else 3, g["M"], g["D"], g["K"], ts)
    g["form"] = expected_form(g["M"], g["D"], g["K"], g["V"], ts, g["streamed"] or g["csr"])
    return g


ROWS_N = (1, 15, 16, 17, 63, 64, 65, 253)
LONG_MFMA = GRID_ROWS_MFMA + 64 + 17            # a second grid-stride pass of 2048 workgroups x 4 waves x 16 rows
LONG_ROWS = GRID_ROWS + 128 + 5                 # ... of 2048 workgroups x 128 rows
GRIDS_M = {3: (3,), 4: (2, 2), 5: (5,), 9: (3, 3), 13: (13,), 16: (4, 4), 17: (17,), 36: (6, 6)}

GROUPS = []
# route 1: rows
GROUPS += [_g(f"mfma-rows-{c}", ctx=c, ns=ROWS_N, n1=37) for c in ("f64", "f32")]
# route 1: inducing points (every residue of M4/4 mod 4 in the rbf64 tail, M4 > M), RBF and the generic branch
GROUPS += [_g(f"mfma-M{M}-{kind}", grid=GRIDS_M[M], kind=kind, modes=(0, 1)) for M in GRIDS_M for kind in ("rbf", "matern32")]
# route 1: topics (NB = 1 and 2)
GROUPS += [_g(f"mfma-K{K}", K=K, n1=21) for K in (1, 4, 5, 15, 16, 17, 31, 32)]
# route 1: vocabulary (the e / V store loop)
GROUPS += [_g(f"mfma-V{V}", V=V, modes=(2, 3)) for V in (1, 7, 64, 65)]
# route 1: D x ARD, DD = 2 and DD = GDRF_DMAX
DGRIDS = {1: (9,), 2: (3, 3), 3: (3, 2, 2), 4: (2, 2, 2, 2)}
GROUPS += [_g(f"mfma-D{D}-{'ard' if ard else 'iso'}-{kind}", D=D, grid=DGRIDS[D], ard=ard, kind=kind, alpha=1.3, K=17 if D == 4 else 5,
              modes=(0, 1))
           for D in (1, 2, 3, 4) for ard in (False, True) for kind in ("rbf", "rationalquadratic")]
# route 1: the float C/D row map, the unwhitened branch
GROUPS += [_g("mfma-pure-K17", ctx="pure", K=17, ns=(65,), n1=37), _g("mfma-pure-K5", ctx="pure", ns=(65,), modes=(0, 1)),
           _g("mfma-f32-K17", ctx="f32", K=17, ns=(65,), modes=(0, 1)),
           _g("mfma-unwhitened", whiten=False, ns=(65,))]
# route 1: a second grid-stride pass
GROUPS += [_g("mfma-long", grid=(5,), K=3, V=3, ns=(LONG_MFMA,), n1=GRID_ROWS_MFMA + 21)]
# routes 2 and 3
RN = (1, 127, 128, 129, 300)
GROUPS += [_g(f"rows-lds-{c}", ctx=c, V="rows_lds", ns=RN, n1=37) for c in ("f64", "f32", "pure")]
GROUPS += [_g(f"rows-mem-{c}", ctx=c, V="rows_mem", ns=RN, n1=37) for c in ("f64", "pure")]
GROUPS += [_g("rows-lds-matern32-ard", kind="matern32", ard=True, V="rows_lds", ns=(129,), modes=(0, 1))]
GROUPS += [_g("rows-lds-long", grid=(5,), K=32, V=230, ns=(LONG_ROWS,), modes=(0, 1), n1=GRID_ROWS + 21)]
# route 4
GROUPS += [_g(f"bigk-K{K}-V{V}", K=K, V=V, ns=(1, 129), n1=37) for K in (33, 64, 65) for V in (3, 11)]
GROUPS += [_g("bigk-K33-f32", ctx="f32", K=33, V=11, ns=(129,))]
GROUPS += [_g("bigk-long", grid=(5,), K=33, V=3, ns=(LONG_ROWS,), modes=(0, 1), n1=GRID_ROWS + 21)]
# route 5
GROUPS += [_g(f"streamed-K{K}-V{V}-{c}", ctx=c, K=K, V=V, ns=(64, 65, 131), n1=37, streamed=True, n_cap=64)
           for (K, V, c) in ((5, 7, "f64"), (40, 70, "f64"), (5, 70, "f32"), (40, 70, "f32"))]
GROUPS += [_g("csr-perplexity", ns=(131,), modes=(3,), csr=True, n_cap=64)]
# mode 4 (predict_var_kernel's 256-thread blocks)
GROUPS += [_g(f"locvar-{c}", ctx=c, ns=(1, 255, 256, 257), modes=(4,), mode4=True, n_cap=257) for c in ("f64", "f32")]
GROUPS += [_g("locvar-unwhitened", whiten=False, ns=(257,), modes=(4,), mode4=True, n_cap=257)]
BY_ID = {g["id"]: g for g in GROUPS}
assert len(BY_ID) == len(GROUPS)


@functools.lru_cache(maxsize=None)
def reference(gid):
    """(inputs, exact, as designed) of a group at its largest n, computed once and shared; nobody writes into them."""
    g = BY_ID[gid]
    inp = make_inputs(g)
    solve, array, _ = CTX[g["ctx"]]
    kw = dict(whiten=g["whiten"], with_var=g["mode4"], need_p=bool({2, 3} & set(g["modes"])))
    exact, designed = restate(inp, g["kind"], LD, LD, **kw), restate(inp, g["kind"], solve, array, **kw)
    for r in (exact, designed):
        for v in r.values():
            v.setflags(write=False)
    return inp, exact, designed


MODE_KEYS = {0: ("loc",), 1: ("theta",), 2: ("p",), 4: ("loc4", "var")}


def exact_output(g, mode, n, key=None):
    """The exact result of (group, mode, n) in the layout gdrf_predict writes (mode 3: the perplexity of its two sums)."""
    inp, exact, _ = reference(g["id"])
    if mode == 3:
        return perplexity(*perp_sums(exact["logp"][:n], inp["ws"][:n]))
    key = key or MODE_KEYS[mode][0]
    return exact[key][:, :n] if key in ("loc", "loc4", "var") else exact[key][:n]


def bound(g, mode, n, key=None):
    """(e_ref, 64 e_ref + floor) of (group, mode, n), from the two restatements alone."""
    inp, exact, des = reference(g["id"])
    array = CTX[g["ctx"]][1]
    if mode == 3:
        e = relerr(perplexity(*perp_sums(des["logp"][:n], inp["ws"][:n])), perplexity(*perp_sums(exact["logp"][:n], inp["ws"][:n])))
        return e, FACTOR * e + FLOOR[np.dtype(np.float64)]              # out_d is float64 in every context type
    key = key or MODE_KEYS[mode][0]
    sl = (slice(None), slice(0, n)) if key in ("loc", "loc4", "var") else (slice(0, n),)
    e = relerr(des[key][sl], exact[key][sl])
    return e, FACTOR * e + FLOOR[np.dtype(array)]
