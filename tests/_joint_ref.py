"""A plain numpy restatement of the joint posterior at new inputs and of the greedy rule's gains (csrc/predict_cov.h, csrc/select_batch.h),
in any numpy dtype; the shapes at which tests/test_gpu_joint_edges.py runs them, the tile sizes those shapes cross, and the error bound of
the all-fp32 context.  CPU only, and the restatement itself is numpy alone; the builders at the end, which hand it a case's numbers, take them
from tests.test_gpu_joint.Case without an engine (torch on the CPU).  tests/test_joint_edges_host.py tests its measures.

    L L^T = K_uu + j_uu I;  W = K_*m L^-T;  R = K_** - W W^T;  T_k = W S_k;  C_k = R + T_k T_k^T;  loc_k = W u_k
    f[s, k] = W (u_k + S_k xi[s, k]) + G zeta[s, k] + mean[k],  G G^T = R + j I        (whiten=False: u_k, S_k are L^-1 u_k, L^-1 S_k)
    d_k[j] = C_k[j][j] - C_k[j, A] (C_k[A, A] + s2 I)^-1 C_k[A, j],  gain[j] = 1/2 sum_k log1p(max(d_k[j], 0) / s2)

K_uu's factor, its inverse and the covariance values are tests/_predict_ref.py's cholesky, lower_inverse and covariance.  G comes from
block_cholesky below, a left-looking factorisation in panels of 32 columns that can leave out the terms a defective chol_kernel would.

The float64 and float32 contexts (solves in float64) keep the float64 torch restatements and the fixed bounds of tests/test_gpu_joint.py
and tests/test_gpu_select_batch.py.  The all-fp32 context follows the protocol of tests/_predict_ref.py: "exact" is this restatement in
np.longdouble, "as designed" the same in float32 throughout, and a quantity passes when
    err(device, exact) <= 64 err(as designed, exact) + 2^-23
with err the measure the GPU tests use for that quantity; the computed bound may never exceed CEILING = 5e-4.  The gains and the
conditional variances take the case's bound for C_k.
"""
import functools

import numpy as np

from tests import _predict_ref as P

LD = P.LD
FACTOR, FLOOR32, CEILING = P.FACTOR, P.FLOOR[np.dtype(np.float32)], P.CEILING["pure"]
TOL = {"fp64": 1e-7, "fp32": 1e-4}             # the fixed bounds of tests/test_gpu_joint.py
CTXS = ("fp64", "fp32", "pure")
TS = {"fp64": 8, "fp32": 8, "pure": 4}         # bytes of a solve-precision element
S2 = 0.37                                      # the noise variance of tests/test_gpu_select_batch.py

# ---- the tile sizes, restated (tests/test_joint_edges_host.py holds them against the headers) ------------------------------------------
MPAD = 32                  # GDRF_MPAD: M is padded to a multiple of it
CHOL_PC = 256              # columns of a staged chunk of chol_kernel's panel update
CHOL_NS = {8: 2, 4: 4}     # NS: strips whose accumulators a wave of chol_kernel carries at once; a strip group is 16 NS strips of 16 rows
CHOL_ROUND = 1024          # rows of one round of chol_kernel's stage (c)
JT = 64                    # GDRF_JT: output tile edge of the joint kernels
SEL_COLS = 16              # GDRF_SEL_COLS: right-hand sides per block of the pass (w_p and 15 topics)
VEC = {8: 2, 4: 4}         # Vec16<TS>::N: elements of a 16-byte vector


def ceil_div(a, b):
    return -(-a // b)


def crossings(ts, M=None, n=None, SK=None, K=None):
    """how often the loops named in the shape lists below run for a solve-precision element of ts bytes"""
    c = {}
    if M is not None:
        mp = c["Mp"] = ceil_div(M, MPAD) * MPAD
        stride = 16 * VEC[ts]                                           # select_pass_kernel: q = gl VE; q < Mp; q += 16 VE
        c["dot_rounds"] = (mp // stride, ceil_div(mp, stride))          # of the last and of the first lane of a lane group
        c["prep_rounds"] = ceil_div(mp, 256)                            # select_prep_kernel's loops over Mp; joint_v_kernel's blocks along Mp
        c["accum_steps"] = mp // (4 * VEC[ts])                          # jt_accum: q += 4 VE
        c["w_tiles"] = ceil_div(mp, JT)                                 # column tiles of W = K_nm L^-T (and of T_k = W S_k)
    if n is not None:
        last = (n - 1) // 32 * 32                                       # the last panel's c0
        c["chol_chunks"] = ceil_div(last, CHOL_PC)                      # pc = 0, CHOL_PC, .. < c0
        c["chol_strip_groups"] = max(1, ceil_div(ceil_div(n - 32, 16), 16 * CHOL_NS[ts])) if n > 32 else 0    # at c0 = 32, the most
        c["chol_rounds"] = ceil_div(n - 32, CHOL_ROUND) if n > 32 else 0                                        # stage (c) at c0 = 0
        c["row_tiles"] = ceil_div(n, JT)
    if SK is not None:
        c["sample_tiles"] = ceil_div(SK, JT)                            # joint_sample_kernel's tiles along (sample, topic)
    if K is not None:
        c["rhs_blocks"] = ceil_div(K, SEL_COLS - 1)                     # nb of select_pass_kernel
    return c


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------
# Inducing points: the first M points of `grid` on [0, span]^D with span = lengthscale x (the widest axis' points - 1), that is a spacing of
# one lengthscale along that axis: every column of W, the last one of a padded block included, then carries a part of the prior variance
# that the measures see (tests/test_joint_edges_host.py zeroes each 32-column block in turn).  Matern-5/2, variance 25.
GRIDS = {(12, 2): (4, 3), (33, 2): (6, 6), (36, 2): (6, 6), (36, 3): (4, 3, 3), (36, 4): (3, 3, 2, 2), (64, 2): (8, 8), (65, 2): (9, 8),
         (257, 2): (17, 16)}
LS = {"fp64": 0.3, "fp32": 0.3, "pure": 0.1}
JITTER = {"fp64": 1e-6, "fp32": 1e-4, "pure": 1e-4}
NS_COV = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)           # tests/test_gpu_joint.py's sweep
NS_SEL = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)                   # tests/test_gpu_select_batch.py's sweep


def _e(id, M, K=3, D=2, kernel="matern52", whiten=True, ns=(65,), ctxs=CTXS, given=0, expect=None, **kw):
    d = dict(id=id, M=M, K=K, D=D, kernel=kernel, whiten=whiten, ns=tuple(ns), ctxs=tuple(ctxs), given=given, grid=GRIDS[(M, D)],
             expect=expect or {})
    d.update(kw)
    return d


# expect: {ts: {crossing: value}} - what the comment claims, recomputed by the host test
COV_CASES = [
    # Mp = 64 with ONE real column in the second block: two rounds of the stride-32 dot product, 8 jt_accum steps in double
    _e("M33", 33, ns=(17, 65, 129), expect={8: dict(Mp=64, accum_steps=8, w_tiles=1), 4: dict(Mp=64, accum_steps=4)}),
    # Mp = 64, the second block full
    _e("M64", 64, ns=(17, 65, 129), expect={8: dict(Mp=64, w_tiles=1)}),
    # Mp = 96: a second column tile of W with half of its columns, an odd number of 32-column blocks
    _e("M65", 65, ns=(17, 65, 129), expect={8: dict(Mp=96, w_tiles=2, accum_steps=12), 4: dict(Mp=96, accum_steps=6)}),
    _e("M65-unwhitened", 65, whiten=False, ns=(17, 65, 129), expect={8: dict(Mp=96)}),
    # Mp = 288, past 256: five column tiles of W, a second block of joint_v_kernel and a second round of 256 threads in select_prep_kernel
    _e("M257", 257, ns=(17, 65, 129), expect={8: dict(Mp=288, w_tiles=5, prep_rounds=2, accum_steps=36), 4: dict(Mp=288, accum_steps=18)}),
    # the GDRF_DMAX = 4 loops of the JT_RESID epilogue with D = 3 and D = 4, isotropic and ARD
    _e("D3", 36, D=3, ns=(17, 65), expect={8: dict(Mp=64)}),
    _e("D4", 36, D=4, ns=(17, 65), expect={8: dict(Mp=64)}),
    _e("D3-ard", 36, D=3, kernel="ard", ns=(17, 65), expect={8: dict(Mp=64)}),
    # the all-fp32 instantiation at every row edge of the product kernel's tiling
    _e("M12-rows", 12, ns=NS_COV, ctxs=("pure",), expect={4: dict(Mp=32, accum_steps=2, w_tiles=1)}),
]
SELECT_CASES = [
    # select_pass_kernel's dot product: 2, 3 and 9 rounds of stride 32 in double; in float the stride is 64: two rounds for lanes 0-7 and
    # one for lanes 8-15 at Mp = 96 (ragged), five and four at Mp = 288
    _e("M33", 33, expect={8: dict(dot_rounds=(2, 2), prep_rounds=1)}, ctxs=("fp64", "fp32")),
    _e("M65", 65, expect={8: dict(dot_rounds=(3, 3), rhs_blocks=1), 4: dict(dot_rounds=(1, 2), rhs_blocks=1)}),
    _e("M257", 257, expect={8: dict(dot_rounds=(9, 9), prep_rounds=2), 4: dict(dot_rounds=(4, 5), prep_rounds=2)}),
    # K + 1 = 16 fills the block of right-hand sides, 17 starts a second one: here with a multi-round dot product
    _e("M65-K15", 65, K=15, expect={8: dict(rhs_blocks=1, dot_rounds=(3, 3))}, ctxs=("fp64", "fp32")),
    _e("M65-K16", 65, K=16, expect={8: dict(rhs_blocks=2, dot_rounds=(3, 3)), 4: dict(rhs_blocks=2, dot_rounds=(1, 2))}),
    _e("M257-K16", 257, K=16, expect={4: dict(rhs_blocks=2, dot_rounds=(4, 5))}, ctxs=("pure",)),
    _e("M65-given5", 65, given=5, expect={8: dict(dot_rounds=(3, 3))}, ctxs=("fp64", "fp32")),
    # the GDRF_DMAX loops of the pass with D = 3, isotropic and ARD
    _e("D3", 36, D=3, expect={8: dict(Mp=64)}, ctxs=("fp64", "fp32")),
    _e("D3-ard", 36, D=3, kernel="ard", expect={8: dict(Mp=64)}, ctxs=("fp64", "fp32")),
    # the all-fp32 instantiation at every row edge of the pass; Mp = 32 leaves lanes 8-15 of each lane group without a round
    _e("M12-rows", 12, ns=NS_SEL, ctxs=("pure",), expect={4: dict(Mp=32, dot_rounds=(0, 1))}),
]
COUNT = 9
# engine-level samples at M = 257 (joint_v_kernel's second block along Mp; whiten=False reads L^-1 u_k and L^-1 S_k)
SAMPLE_M_CASES = [
    _e("M257-whitened", 257, K=2, S=3, expect={8: dict(prep_rounds=2)}),
    _e("M257-unwhitened", 257, K=2, S=3, whiten=False, expect={8: dict(prep_rounds=2)}),
]
PHILOX_CASE = _e("M257-philox", 257, K=3, S=43, expect={8: dict(prep_rounds=2, sample_tiles=3)})     # S K = 129
# model-level samples, M = 20 on the (5, 4) grid of tests/test_gpu_joint.py's model_case.  n:
#   288   the last panel is c0 = 256: the first chunk of chol_kernel's panel update, full, and no second one
#   289   c0 = 288: the second chunk
#   545   n - 32 = 513 rows below the first panel: 33 strips, a second strip group in double (NS = 2, 32 strips a group)
#   1057  n - 32 = 1025: 65 strips, a second strip group in float (NS = 4); stage (c)'s second round of 1024 rows
SAMPLE_N = {"fp64": (288, 289, 545, 1057), "fp32": (288, 289, 545, 1057), "pure": (289, 1057)}
SAMPLE_N_EXPECT = {
    288: {8: dict(chol_chunks=1, chol_strip_groups=1, chol_rounds=1)},
    289: {8: dict(chol_chunks=2, chol_strip_groups=1, chol_rounds=1), 4: dict(chol_chunks=2)},
    545: {8: dict(chol_chunks=3, chol_strip_groups=2, chol_rounds=1), 4: dict(chol_strip_groups=1)},
    1057: {8: dict(chol_chunks=5, chol_strip_groups=3, chol_rounds=2), 4: dict(chol_chunks=5, chol_strip_groups=2, chol_rounds=2)},
}
# the large-n samples of the all-fp32 context need the rows' jitter at 0.1 and a lengthscale of 0.05 to stay under the ceiling
# and the last row is a twin of the one before it, TWIN = a tenth of a lengthscale away: at n = 289 the second chunk of the panel update
# holds nothing but that row's 32 terms, which then carry nearly all of its variance
MODEL_LS = {"fp64": 0.05, "fp32": 0.05, "pure": 0.05}
TWIN = 0.005
MODEL_JITTER = {"fp64": 1e-6, "fp32": 1e-4, "pure": 0.1}
MODEL_GRID = (5, 4)
# (K, S) at n = 33: S K = 63, 129 (K = 3) and 64, 65 (K = 1) - one tile of joint_sample_kernel short of a row, full, a second tile of one
# row, a third tile of one row
SAMPLE_SK = ((3, 21), (3, 43), (1, 64), (1, 65))
SAMPLE_SK_EXPECT = {63: 1, 64: 1, 65: 2, 129: 3}
SAMPLE_SK_N = 33


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def make_inputs(kernel, Z, X, log_ls, log_var, u, s_unc, whiten, jitter, xi=None, zeta=None, mean=None, jrow=None):
    """float64 arrays holding the values the context holds (float32-valued in the float32 context types)"""
    a = lambda v: None if v is None else np.asarray(v, dtype=np.float64)
    return dict(kind="rbf" if kernel == "ard" else kernel, Z=a(Z), X=a(X), log_ls=a(log_ls), log_var=float(log_var), u=a(u), s_unc=a(s_unc),
                whiten=bool(whiten), jitter=float(jitter), xi=a(xi), zeta=a(zeta), mean=a(mean), jrow=None if jrow is None else float(jrow))


def _chol_diag(A):
    """lower factor of a block of at most 32 columns by a column loop, in A's dtype; a pivot <= 0 is flagged and replaced by 1, as the
    kernel does"""
    m = A.shape[0]
    L = np.zeros_like(A)
    bad = False
    for j in range(m):
        d = A[j, j] - np.sum(L[j, :j] * L[j, :j], dtype=A.dtype)
        if not d > 0:
            bad, d = True, A.dtype.type(1)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]).sum(1, dtype=A.dtype)) / L[j, j]
    return L, bad


def block_cholesky(A, drop=None, ts=8):
    """(lower factor, a pivot failed) of A in its dtype: left-looking in panels of 32 columns, as chol_kernel orders it.  drop leaves out
    what a defective kernel would:  "chunk"  the panel update's terms past its first CHOL_PC columns;  "strips"  the update of the rows
    past the first strip group (16 CHOL_NS[ts] strips of 16 rows);  "round"  stage (c) for the rows past its first CHOL_ROUND"""
    n = A.shape[0]
    L = np.tril(A).copy()
    bad = False
    for c0 in range(0, n, 32):
        c1 = min(c0 + 32, n)
        if c0:
            q1 = min(c0, CHOL_PC) if drop == "chunk" else c0
            r1 = min(n, c0 + 16 * 16 * CHOL_NS[ts]) if drop == "strips" else n
            L[c0:r1, c0:c1] -= L[c0:r1, :q1] @ L[c0:c1, :q1].T
        Ld, b = _chol_diag(L[c0:c1, c0:c1])
        bad = bad or b
        L[c0:c1, c0:c1] = Ld
        r1 = min(n, c1 + CHOL_ROUND) if drop == "round" else n
        if c1 < r1:
            L[c1:r1, c0:c1] = L[c1:r1, c0:c1] @ P.lower_inverse(Ld).T
    return np.tril(L), bad


def restate(inp, t, zero_block=None, drop=None, ts=8, picks=None, given=0, s2=S2):
    """every checked quantity of the inputs in the dtype t:  W (n, M), loc (K, n), R (n, n), C (K, n, n);  f (S, K, n) where xi and zeta are
    given (G from R + jrow I; "chol_failed");  gain0 (n,) the gains before any pick and, where `picks` is given, dvar (K, n) the
    conditional variances after the `given` trailing rows and the picks.  zero_block b: W[:, 32 b : 32 b + 32] is zeroed before anything
    reads W - what a loop over Mp that skips that block computes.  drop: see block_cholesky."""
    hp = np.float64 if np.finfo(t).bits <= 64 else t
    Z, X = inp["Z"], inp["X"]
    M, D = Z.shape
    ls = np.exp(np.atleast_1d(inp["log_ls"]).astype(hp)) * np.ones(D, dtype=hp)
    var = np.exp(hp(inp["log_var"]))
    cov = lambda A, B: P.covariance(inp["kind"], A, B, ls, var, 1.0, t)
    Linv = P.lower_inverse(P.cholesky(cov(Z, Z) + t(inp["jitter"]) * np.eye(M, dtype=t)))
    W = cov(X, Z) @ Linv.T
    if zero_block is not None:
        W[:, 32 * zero_block:32 * zero_block + 32] = 0
    s_unc = inp["s_unc"]
    S = (np.tril(s_unc, -1) + np.exp(np.diagonal(s_unc, axis1=1, axis2=2).astype(hp))[:, :, None] * np.eye(M)).astype(t)
    u = inp["u"].astype(t)
    if not inp["whiten"]:
        u, S = u @ Linv.T, Linv[None] @ S
    R = cov(X, X) - W @ W.T
    T = W[None] @ S
    out = dict(W=W, loc=u @ W.T, R=R, C=R[None] + T @ T.transpose(0, 2, 1))
    if inp["xi"] is not None:
        n = X.shape[0]
        G, out["chol_failed"] = block_cholesky(R + t(inp["jrow"]) * np.eye(n, dtype=t), drop, ts)
        v = u[None] + (S[None] @ inp["xi"].astype(t)[..., None])[..., 0]                # (S, K, M)
        f = v @ W.T + inp["zeta"].astype(t) @ G.T
        out["f"] = f if inp["mean"] is None else f + inp["mean"].astype(t)[None]
        if inp["mean"] is not None:
            out["f0"] = out["loc"] + inp["mean"].astype(t)                                # the sample of an all-zero draw
    # the batch choice: d starts as mode 4's variance, clamp included
    diag = np.maximum(t(var) - (W * W).sum(1, dtype=t), t(0))[None] + (T * T).sum(2, dtype=t)         # (K, nt)
    nc = X.shape[0] - given
    gain = lambda d: (t(0.5) * np.log1p(np.maximum(d, t(0)) / t(s2))).sum(0, dtype=t)[:nc]
    out["gain0"], out["diag"] = gain(diag), diag
    if picks is not None:
        A = list(range(nc, nc + given)) + [int(p) for p in picks]
        dvar = diag.copy()
        for k in range(S.shape[0]):
            CA = out["C"][k][:, A]                                                      # (nt, |A|)
            Li = P.lower_inverse(P.cholesky(CA[A, :] + t(s2) * np.eye(len(A), dtype=t)))
            Y = Li @ CA.T
            dvar[k] -= (Y * Y).sum(0, dtype=t)
        out["dvar"], out["gain_last"] = dvar[:, :nc], gain(dvar)
    return out


def greedy_picks(q, count, given=0, s2=S2):
    """the greedy rule's picks on restate's result q (float64 dense solves; ties to the lower index)"""
    C, diag = np.asarray(q["C"], dtype=np.float64), np.asarray(q["diag"], dtype=np.float64)
    nc = C.shape[1] - given
    A, picks = list(range(nc, nc + given)), []
    for _ in range(count):
        d = diag.copy()
        if A:
            for k in range(C.shape[0]):
                CA = C[k][:, A]
                d[k] -= (CA * np.linalg.solve(CA[A, :] + s2 * np.eye(len(A)), CA.T).T).sum(1)
        g = 0.5 * np.log1p(np.maximum(d, 0.0) / s2).sum(0)[:nc]
        g[picks] = -np.inf
        picks.append(int(np.argmax(g)))
        A.append(picks[-1])
    return picks


def measures(got, ref):
    """the GPU tests' measure of each quantity both hold: C and f relative to their own largest magnitude, R relative to max |C| (it nearly
    vanishes near the inducing points), the gains relative to the largest first gain, the variances relative to the largest prior variance"""
    m = {}
    scale = {"C": "C", "R": "C", "f": "f", "f0": "f0", "loc": "loc", "gain0": "gain0", "gain_last": "gain0", "dvar": "diag"}
    for k, s in scale.items():
        if k in got and k in ref:
            a, b = np.asarray(got[k], dtype=LD), np.asarray(ref[k], dtype=LD)
            m[k] = float(np.abs(a - b).max() / np.abs(np.asarray(ref[s], dtype=LD)).max()) if np.isfinite(a.astype(np.float64)).all() else float("inf")
    return m


def pure_bounds(designed, exact):
    """{quantity: 64 err(as designed, exact) + 2^-23}; the gains and the variances take C's"""
    b = {k: FACTOR * e + FLOOR32 for k, e in measures(designed, exact).items()}
    for k in ("gain0", "gain_last", "dvar"):
        b[k] = b["C"]
    return b


@functools.lru_cache(maxsize=None)
def _pure_reference(key, maker):
    inp, kw = maker(*key)
    exact, designed = restate(inp, LD, **kw), restate(inp, np.float32, ts=4, **kw)
    for r in (exact, designed):
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return inp, exact, pure_bounds(designed, exact)


def pure_reference(maker, *key):
    """(inputs, exact, bounds) of the all-fp32 case maker(*key) -> (inputs, restate's keywords); computed once and shared, nobody writes into them"""
    return _pure_reference(key, maker)


# ---- the cases' numbers: tests.test_gpu_joint.Case without an engine (torch on the CPU; imported here and not above, so that the
# restatement itself stays plain numpy) ---------------------------------------------------------------------------------------------------

def torch_dtype(ctx):
    import torch
    return torch.float64 if ctx == "fp64" else torch.float32


def make_case(e, ctx, n_cap=129, engine=False):
    """the tests.test_gpu_joint.Case of an entry of the lists above in a context type"""
    import tests.test_gpu_joint as J
    ls = LS[ctx]
    return J.Case(e["kernel"], e["M"], e["K"], torch_dtype(ctx), whiten=e["whiten"], n_cap=n_cap, jitter=JITTER[ctx], ls=ls, D=e["D"],
                  grid=e["grid"], span=ls * (max(e["grid"]) - 1), pure=ctx == "pure", engine=engine)


def case_inputs(case, X, **kw):
    return make_inputs(case.kernel, case.Z, X, case.hyp["log_lengthscale"], case.hyp["log_variance"], case.u, case.s_unc, case.whiten,
                       case.jitter, **kw)


def normals(S, K, M, n, dtype, seed=3):
    """injected (xi, zeta) of a sample case, values the dtype holds exactly"""
    import torch
    import tests.test_gpu_joint as J
    g = torch.Generator().manual_seed(seed + 1000 * S + n)
    return (J.rnd(torch.randn(S, K, M, generator=g, dtype=torch.float64), dtype), J.rnd(torch.randn(S, K, n, generator=g, dtype=torch.float64), dtype))


def _list(name):
    return {e["id"]: e for e in {"cov": COV_CASES, "select": SELECT_CASES, "sample": SAMPLE_M_CASES}[name]}


def engine_inputs(name, id, ctx, n):
    """(inputs, restate's keywords) of the entry `id` of a list at n rows: the rows are Case.rows(n, 1), the first seed of
    rows_with_a_gap (followed by the entry's given rows), the normals those of normals()"""
    e = _list(name)[id]
    case = make_case(e, ctx)
    X, kw = case.rows(n, 1), {}
    if e["given"]:
        import torch
        X, kw = torch.cat([X, case.rows(e["given"], seed=77, near=False)]), dict(given=e["given"])
    extra = {}
    if name == "sample":
        xi, zeta = normals(e["S"], e["K"], e["M"], n, case.dtype)
        extra = dict(xi=xi, zeta=zeta, jrow=case.jitter)
    return case_inputs(case, X, **extra), kw


def model_hyp(ctx):
    """(log lengthscale, log variance) the model-level cases load: values the context's element type holds"""
    import torch
    import tests.test_gpu_joint as J
    lg = lambda v: J.rnd(torch.as_tensor(v, dtype=torch.float64).log(), torch_dtype(ctx))
    return lg(MODEL_LS[ctx]), lg(25.0)


def model_inputs(K, S, n, ctx):
    """(inputs, restate's keywords) of the model-level sample case: model_case's rows, u and S on its (5, 4) grid, Matern-5/2, the mean
    function's values as the context's element type computes them"""
    import tests.test_gpu_joint as J
    dtype = torch_dtype(ctx)
    xs, _, u, s_unc = J.model_numbers(K, n, dtype, twin=TWIN)
    Z = J.rnd(J.grid_points(MODEL_GRID, int(np.prod(MODEL_GRID))), dtype)
    xi, zeta = normals(S, K, u.shape[1], n, dtype)
    ll, lv = model_hyp(ctx)
    mean = J.mean_fn(K)(xs.to(dtype)).double()
    j = MODEL_JITTER[ctx]
    return make_inputs("matern52", Z, xs, ll, lv, u, s_unc, True, j, xi=xi, zeta=zeta, mean=mean, jrow=j), {}
