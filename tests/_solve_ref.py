"""The solve side of a step - K_nm in the solve precision, W = K_nm L^-T with its row norms q, and the backward through K_nm - restated in
plain numpy, with the table of shapes at which tests/test_gpu_solve_edges.py runs it and a DERIVED error bound for every output.  CPU only:
numpy with np.longdouble, no engine import.

Every reference takes the engine's OWN buffers as inputs (the rows X and inducing inputs Z as stored, the stored parameters, and the
workspaces Knm, Linv, W, Wbar read back from the device), so that only the arithmetic of the stage under test differs:

  K_nm     k(x_n, z_j) from the direct (x - z)^2 form in long double; pyro's r = sqrt(r2 + 1e-12) for the Matern and Exponential kinds; ARD by
           scaled coordinates; Periodic and Product by the closed formula var exp(-2 sum sin^2(pi (x - z) / p) / ls^2 - sum (x - z)^2 / 2 ls^2).
           Hyper-parameters: exp in double of the stored parameters (what prep_hyper*_kernel does).
  W        Knm_got Linv_got^T.
  q        row sums of W_got^2 (W as stored, cast up); also bounded against the row sums of (Knm_got Linv_got^T)^2, since the device takes
           the partial sums from its accumulators before W is stored.
  Kbar     Wbar_got Linv_got (never stored by the device), and from it and Knm_got the sums the backward leaves in red_d:
             red_d[4] = sum Kbar K,  red_d[5] = sum Kbar dK/dlog(ls),  red_d[6] = sum Kbar dK/dlog(alpha)  (RationalQuadratic only),
             learn_inducing: red_d[8 + j D + d] = G[j][d] = sum_n Kbar[n][j] dk/dr2 (z_jd - x_nd),
             ARD / Periodic / Product: behind G, the per-coordinate sums  sum Kbar dk/dr2 (-2) (x_d - z_d)^2  and, per Periodic axis,
             sum Kbar dk/dr2 (-2) (t x - t z) sin(t x - t z) / ls^2  (t = 2 pi / period); all in the coordinates the kernels see (scaled by 1 / ls_d).
  G^T      W_got^T Wbar_got.

BOUNDS.  First-order rounding bounds from the operands' magnitudes, returned with every reference; u = the unit roundoff of the type the
device accumulates in (2^-53 for the f64 solve, 2^-24 for pure_fp32 contexts).
  dot products   gamma(k) (|A| |B|^T) elementwise, gamma(k) = C_MFMA (k + 2) u with k the reduction length (Mp) and C_MFMA = 4 for the matrix
                 instruction's internal order (four k indices per instruction, accumulated in an unspecified order), plus one u of the output
                 type where the result is stored narrower than it was accumulated (the float32 W of the f64 solve).
  sums           sum (bound of Kbar) |dK|  +  (gamma(SUM_TERMS) + C_TERM(D) u) sum |Kbar| |dK|:  a lane adds at most SUM_TERMS = 64 products in the
                 solve precision before the partial sums meet in double; C_TERM = D + 12 roundings go into one term (D + 2 for the recomputed r2,
                 at most 8 for the derivative factor from the stored k, 2 for the products; every factor's log-derivative in r2 is at most 1).
  K_nm, RBF in double (knm_rbf_f64_kernel: k = 2^t, t = log2 var - sum_d (a x_d - a z_d)^2, a = sqrt(log2 e / 2) / ls):  per coordinate the two
                 products a x, a z (u (|a x| + |a z|)), the difference (u |dd|) and the rounding of a itself (2 u |dd|) give the error of dd; the D
                 fused multiply-adds add 2 |dd| err(dd) + u |t| each and log2 var adds u |log2 var|;  err(k) = k (ln 2 err(t) + 1.7e-16 + 4 u):
                 the degree-12 polynomial's remainder and its Horner steps.
  K_nm, generic kernel:  k ((D + 2 + C_ARG) u |dlog k / dlog r2| + C_PROFILE u):  (D + 2) u on r2 and 4 u for the evaluation of the profile
                 (exp, the products with the variance) are the base, which is all of it for RBF.  The other profiles round more, counted from
                 cov_from_r2 (csrc/common.h), every rounding of the profile's ARGUMENT as its equivalent on r2:
                   Exponential  r = sqrt(r2 + 1e-12): the sum 1 u on r2, the root 1 u on r = 2 u on r2: C_ARG = 3;
                   Matern-3/2   as above, and a = sqrt(3) r: the rounded constant and the product, 1 u on r each = 4 u on r2: C_ARG = 7;
                   Matern-5/2   C_ARG = 7, and the polynomial 1 + a + (5/3) r r adds the rounded 5/3, two products and two sums, each at
                                most 1 u of the polynomial: C_PROFILE = 4 + 4 = 8;
                   RationalQuadratic  r2 (0.5 / alpha): the quotient and the product: C_ARG = 2; 1 + . moves the logarithm by u, the logarithm
                                and its product with alpha round |log(k / var)| u each: C_PROFILE = 2 + alpha + 2 |log(k / var)|, at least 4.
  float32 underflow (pure_fp32): a float32 result below the smallest normal number 2^-126 loses bits or is flushed to zero: an absolute
                 2^-126 per product or element on top of every bound of that context type.
  hyper-parameters:  the device's exp and the host's may differ in the last place, and 1 / ls^2 adds two roundings: 2 u64 on the variance and
                 6 u64 on r2, in every context; pure_fp32 contexts round the double block to float32: one more u on each.
  rounded inputs:  the coordinates the device rounds before the stage (the scaled inducing inputs and rows of ARD contexts: one roundoff of
                 their stored type; the embedded coordinates of periodic contexts: (|t x| + 3) u / ls for the rounding of the phase, of sin / cos
                 and of the stored value) count as an input perturbation: 2 |dd| (pert_x + pert_z) on r2, through |dk / dr2|.
  hyper_backward="tn":  red_d[4] = sum Wbar W on the stored W: the bound of W through |Wbar|;  red_d[5] through Hd = dK^T Wbar on the split
                 fp16 kernel: SPLIT_TOL max |Hd| (what tests/test_gpu_topic_forms.py holds G^T on the same kernel to) times sum |L^-1|.
  G^T            f64: gamma(n) |W|^T |Wbar|;  float32 arrays: SPLIT_TOL max |G^T| in addition (the same kernel, the same file's bound).
No constant here was tuned to a measured value; DESIGN.md ("Testing notes of the solve side") records what the MI355X gave.

DATA.  Inducing inputs in random order (every column tile then holds points from the whole domain), lengthscale 2 M^(-1/D) (about two
spacings: no tile of W is negligible and K_uu + jitter factorises in float32), variance 1.5, cumulative jitter 1.1e-2 (level 1 of a 1e-3
schedule).  Row 0 sits exactly on z_0 (r2 = 0: the 1e-12 under the root is then visible) and the last row half a lengthscale from z_(M-1), or at the
centre of the domain where it is a row tile of its own (the most neighbours in every column tile), and the counts of the last, ragged row
tile are scaled 20x, as tests/test_gpu_topic_forms.py does; u_loc is 6x on a last column tile of at most 8 columns.
"""
import functools
import math

import numpy as np

LD = np.longdouble
HAS_LONGDOUBLE = bool(np.finfo(LD).eps < 1e-18)
KINDS = ("rbf", "matern52", "matern32", "exponential", "rationalquadratic")
TILE = 128
U64, U32 = 2.0 ** -53, 2.0 ** -24
C_MFMA, SUM_TERMS, POLY_REMAINDER = 4.0, 64, 1.7e-16
TINY32 = 2.0 ** -126
C_ARG = dict(rbf=0, periodic=0, product=0, exponential=3, matern32=7, matern52=7, rationalquadratic=2)
SPLIT_TOL = 2e-6                      # tests/test_gpu_topic_forms.py: GLOBAL["split"]["GT"]
JITTER, LEVEL = 1e-3, 1
JITTER_TOTAL = JITTER + 10 * JITTER   # Engine.jitter_total(1)
VARIANCE, NOISE, ALPHA = 1.5, 0.5, 1.3
MIN_SHARE = 1e-3


def c_term(D):
    return D + 12.0


def gamma(k, u):
    return C_MFMA * (k + 2) * u


# ---- the cases --------------------------------------------------------------------------------------------------------------------------

def _case(ctx, kind, M, n, D, edges, K=2, **opts):
    return dict(ctx=ctx, kind=kind, M=M, n=n, D=D, K=K, V=6, n_cap=opts.pop("n_cap", n), opts=opts, edges=tuple(edges))


# ctx: "f64" (float64 arrays), "f32" (float32 arrays, f64 solve), "pure" (pure_fp32).  opts: learn_inducing, ard, hyper_tn, mfma_mode, n_cap,
# periodic (one Periodic factor over the D raw axes) / product (Periodic on axis 0 x RBF on axis 1).  edges: what the case claims to cross;
# tests/test_solve_edges_host.py recomputes each from the shapes.
CASES = {
    # fp64: every M, n, D and kind.  The one-row last tiles (n = 129, 1025) meet M = 5, 33, 250, 512 and the one-column last tiles (M = 65, 129,
    # 257, 513) meet n = 1, 127, 128: a tile of ONE term cannot carry 1e-3 of a sum of n M terms, whatever the data
    "f64_rbf_M5_n1_D1": _case("f64", "rbf", 5, 1, 1, ("M5", "n1", "D1")),
    "f64_m52_M33_n129_D2": _case("f64", "matern52", 33, 129, 2, ("M33", "n129", "D2", "root", "ragged", "rmax")),
    "f64_m32_M65_n128_D3": _case("f64", "matern32", 65, 128, 3, ("M65", "n128", "D3", "root")),
    "f64_exp_M129_n127_D4": _case("f64", "exponential", 129, 127, 4, ("M129", "n127", "D4", "root", "ragged")),
    "f64_rq_M250_n1025_D2": _case("f64", "rationalquadratic", 250, 1025, 2, ("M250", "n1025", "serpentine", "round2", "ragged", "rmax", "tri1", "tri2")),
    "f64_rbf_M257_n127_D2": _case("f64", "rbf", 257, 127, 2, ("M257", "rpp1", "ragged", "rmax")),
    "f64_rbf_M512_n129_D2": _case("f64", "rbf", 512, 129, 2, ("M512", "n129", "serpentine", "tri1", "tri2", "ragged", "rmax")),
    "f64_rbf_M513_n127_D2": _case("f64", "rbf", 513, 127, 2, ("M513", "wide_rows")),
    "f64_m52_M513_n128_D3": _case("f64", "matern52", 513, 128, 3, ("M513", "wide_rows")),
    "f64_rbf_M65_n127_D3": _case("f64", "rbf", 65, 127, 3, ("M65", "idle_threads", "rbf_dd4")),
    "f64_rbf_M250_n1025_D4": _case("f64", "rbf", 250, 1025, 4, ("M250", "rbf_dd4", "n_cap", "tri1", "round2"), n_cap=1100),
    "f64_rq_M33_n1_D3": _case("f64", "rationalquadratic", 33, 1, 3, ("n1", "D3")),
    "f64_exp_M5_n1025_D1": _case("f64", "exponential", 5, 1025, 1, ("M5", "n1025", "round2", "n_cap", "root"), n_cap=1100),
    "f64_m32_M257_n128_D1": _case("f64", "matern32", 257, 128, 1, ("M257", "n128", "D1")),
    "f64_rbf_M129_n127_D2_K1": _case("f64", "rbf", 129, 127, 2, ("M129", "K1"), K=1),
    # float32 arrays, f64 solve: the W epilogue through LDS with the pieces of the split modes
    "f32_rbf_M250_n1025_D2": _case("f32", "rbf", 250, 1025, 2, ("serpentine", "round2", "f16x3", "tri1", "tri2")),
    "f32_m52_M65_n127_D2": _case("f32", "matern52", 65, 127, 2, ("M65", "f16x3", "ragged", "rmax")),
    "f32_rbf_M512_n128_D3": _case("f32", "rbf", 512, 128, 3, ("M512", "rbf_dd4", "f16x3")),
    "f32_exp_M129_n127_D1": _case("f32", "exponential", 129, 127, 1, ("M129", "n_cap", "f16x3"), n_cap=131),
    "f32_rq_M33_n129_D4": _case("f32", "rationalquadratic", 33, 129, 4, ("M33", "D4", "f16x3")),
    "f32_m32_M513_n128_D2": _case("f32", "matern32", 513, 128, 2, ("M513", "wide_rows", "f16x3")),
    "bf16_rbf_M129_n127_D2": _case("f32", "rbf", 129, 127, 2, ("bf16x6",), mfma_mode="bf16x6"),
    "bf16_m52_M250_n1025_D3": _case("f32", "matern52", 250, 1025, 3, ("bf16x6", "round2"), mfma_mode="bf16x6"),
    # pure_fp32: the f32 solve (128-wide column tiles, 32-deep chunks)
    "pure_rbf_M5_n1_D2": _case("pure", "rbf", 5, 1, 2, ("pure", "n1")),
    "pure_m52_M129_n127_D2": _case("pure", "matern52", 129, 127, 2, ("pure", "ragged")),
    "pure_rbf_M512_n1025_D2": _case("pure", "rbf", 512, 1025, 2, ("pure", "serpentine32", "round2", "tri1")),
    "pure_exp_M257_n127_D3": _case("pure", "exponential", 257, 127, 3, ("pure",)),
    "pure_rq_M65_n128_D4": _case("pure", "rationalquadratic", 65, 128, 4, ("pure",)),
    "pure_m32_M513_n128_D1": _case("pure", "matern32", 513, 128, 1, ("pure", "M513")),
    # learnable inducing inputs: the generic epilogue even at D <= 2, G[j][d]
    "lz_f64_rbf_M65_n127_D2": _case("f64", "rbf", 65, 127, 2, ("lz", "ragged"), learn_inducing=True),
    "lz_f64_m52_M250_n1025_D1": _case("f64", "matern52", 250, 1025, 1, ("lz", "serpentine", "round2", "ragged"), learn_inducing=True),
    "lz_f32_rq_M129_n127_D3": _case("f32", "rationalquadratic", 129, 127, 3, ("lz",), learn_inducing=True),
    "lz_pure_m32_M250_n129_D2": _case("pure", "matern32", 250, 129, 2, ("lz", "pure", "tri2"), learn_inducing=True),
    # ARD, with and without learnable inducing inputs
    "ard_f64_rbf_M129_n127_D2": _case("f64", "rbf", 129, 127, 2, ("ard", "ragged", "rmax"), ard=True),
    "ard_f64_m52_M65_n127_D3": _case("f64", "matern52", 65, 127, 3, ("ard",), ard=True),
    "ard_lz_f64_rbf_M33_n129_D4": _case("f64", "rbf", 33, 129, 4, ("ard", "lz", "ragged"), ard=True, learn_inducing=True),
    "ard_f32_exp_M250_n129_D2": _case("f32", "exponential", 250, 129, 2, ("ard",), ard=True),
    "ard_pure_rq_M65_n127_D2": _case("pure", "rationalquadratic", 65, 127, 2, ("ard", "pure"), ard=True),
    # Periodic and Product, fp64
    "per_f64_M65_n127_D1": _case("f64", "periodic", 65, 127, 1, ("periodic", "ragged", "rmax")),
    "prod_f64_M129_n127_D2": _case("f64", "product", 129, 127, 2, ("product", "ragged")),
    # the hyper-TN alternative (float32 arrays, f16x3, fixed inducing inputs)
    "tn_f32_rbf_M513_n127_D2": _case("f32", "rbf", 513, 127, 2, ("hyper_tn", "dk_rpp3"), hyper_tn=True),
    "tn_f32_m52_M250_n1025_D2": _case("f32", "matern52", 250, 1025, 2, ("hyper_tn", "round2"), hyper_tn=True),
}

PRODUCT_TABLE = [dict(name="kern0", kind="periodic", active_dims=[0], lengthscales=1, periods=1),
                 dict(name="kern1", kind="rbf", active_dims=[1], lengthscales=1, periods=0)]


def solve_dtype(case):
    return np.float32 if case["ctx"] == "pure" else np.float64


def array_dtype(case):
    return np.float64 if case["ctx"] == "f64" else np.float32


def facts(case):
    """What the host derives from the shapes of a case (csrc/api.hip, gemm_nt.h, kernels_n.h, hyper_tn.h)."""
    M, n, n_cap = case["M"], case["n"], case["n_cap"]
    Mp = (M + 31) // 32 * 32
    f32 = case["ctx"] == "pure"
    cw, bk, ve = (128, 32, 4) if f32 else (64, 16, 2)
    nct = -(-Mp // cw)
    rtiles = -(-n // TILE)
    vpr = Mp // ve
    kernel_d = coord_count(case)
    return dict(Mp=Mp, cw=cw, bk=bk, nct=nct, rtiles=rtiles, grid=8 * nct * (-(-rtiles // 8)), padding_blocks=8 * nct * (-(-rtiles // 8)) - nct * rtiles,
                serpentine=nct % 4 == 0, round2=rtiles > 8, last_rows=n - (rtiles - 1) * TILE, vpr=vpr, wide_rows=vpr > 256,
                rpp=(256 // vpr if vpr <= 256 else 1), idle_threads=(vpr <= 256 and 256 % vpr != 0),
                rbf_f64=(not f32 and case["kind"] in ("rbf", "periodic", "product") and vpr <= 256), dd=2 if kernel_d <= 2 else 4,
                half_tile=(Mp % cw) != 0, ke_capped=nct * cw > Mp, ldk=(n_cap + 3) // 4 * 4, dk_rpp=256 // (Mp // 8) if Mp // 8 <= 256 else 0,
                last_chunk_valid=M > Mp - bk, D=kernel_d,
                epilogue=("lds" if (not f32 and kernel_d <= 2 and not case["opts"].get("learn_inducing")) else "generic"))


def coord_count(case):
    """Coordinates the covariance kernels see: the raw axes, or the embedded ones of periodic / product contexts."""
    if case["kind"] == "periodic":
        return 2 * case["D"]
    if case["kind"] == "product":
        return 3
    return case["D"]


def sources(case):
    """Periodic / product contexts: (raw axis, is a pair, name of its log-lengthscale, name of its log-period), pairs first (CoordTab)."""
    if case["kind"] == "periodic":
        return [(d, True, "log_lengthscale", "log_period") for d in range(case["D"])]
    if case["kind"] == "product":
        return [(0, True, "kern0.log_lengthscale", "kern0.log_period"), (1, False, "kern1.log_lengthscale", None)]
    return None


def inputs(name):
    """Inducing inputs, rows, counts, noise draws and the unconstrained parameters of a case (numpy, fp64 values)."""
    case = CASES[name]
    M, n, D, K, V = case["M"], case["n"], case["D"], case["K"], case["V"]
    rng = np.random.default_rng(sum(name.encode()) + 7 * M + n)
    Z = 0.05 + 0.9 * rng.random((M, D))
    X = rng.random((n, D))
    ls = 2.0 * M ** (-1.0 / D)
    f = facts(case)
    X[0] = Z[0]
    X[n - 1] = 0.5 if f["last_rows"] == 1 and n > 1 else Z[M - 1] + 0.5 * ls / math.sqrt(D)
    ws = rng.integers(0, 6, size=(n, V))
    ws[(n - 1) // TILE * TILE:] *= 20
    u = 0.3 * rng.standard_normal((K, M))
    last0 = (f["nct"] - 1) * f["cw"]
    if M - last0 <= 8:                   # a last column tile of a few columns: their u_loc 6x, so that W-bar is not small there
        u[:, last0:] *= 6
    s = np.tril(0.02 * rng.standard_normal((K, M, M)), -1)
    s[:, np.arange(M), np.arange(M)] = np.log(0.5)
    params = dict(log_variance=math.log(VARIANCE), log_noise=math.log(NOISE), u_loc=u, u_scale_tril_unc=s, phi_unc=0.5 * rng.standard_normal((K, V)))
    if case["kind"] == "product":
        del params["log_variance"]
        params.update({"kern0.log_variance": math.log(1.2), "kern1.log_variance": math.log(VARIANCE / 1.2), "kern0.log_lengthscale": math.log(0.3),
                       "kern0.log_period": math.log(0.37), "kern1.log_lengthscale": math.log(ls)})
    elif case["kind"] == "periodic":
        params.update(log_lengthscale=math.log(0.15), log_period=math.log(0.37))
    elif case["opts"].get("ard"):
        params["log_lengthscale"] = np.log(ls * (1.0 + 0.25 * np.arange(D)))
    else:
        params["log_lengthscale"] = math.log(ls)
    if case["kind"] == "rationalquadratic":
        params["log_scale_mixture"] = math.log(ALPHA)
    return dict(Z=Z, X=X, ws=ws.astype(np.int32), eps=rng.standard_normal((K, n)), params=params)


def stored(d, case):
    """The inputs as the context stores them: rounded to the array type, as float64 values."""
    t = array_dtype(case)
    r = lambda v: np.asarray(v, np.float64).astype(t).astype(np.float64)
    return dict(Z=r(d["Z"]), X=r(d["X"]), params={k: r(v) for k, v in d["params"].items()})


# ---- K_nm -------------------------------------------------------------------------------------------------------------------------------

def profile(kind, r2, var, alpha, t=LD, root_eps=True):
    """k and the factors dk/dlog(ls) / k, dk/dr2 / k, dk/dlog(alpha) / k at r2 = squared distance / ls^2, in dtype t (csrc/common.h)."""
    r2 = np.asarray(r2, dtype=t)
    var, alpha = t(var), t(alpha)
    one, zero = np.ones_like(r2), np.zeros_like(r2)
    if kind in ("rbf", "periodic", "product"):
        return var * np.exp(-r2 / t(2)), r2, -one / t(2), zero
    if kind == "rationalquadratic":
        uu = r2 / (t(2) * alpha)
        den = one + uu
        return var * np.exp(-alpha * np.log1p(uu)), r2 / den, -one / (t(2) * den), alpha * (uu / den - np.log1p(uu))
    r = np.sqrt(r2 + (t(1e-12) if root_eps else t(0)))
    r = np.where(r > 0, r, t(1e-300))
    if kind == "exponential":
        return var * np.exp(-r), r2 / r, -one / (t(2) * r), zero
    if kind == "matern32":
        a = np.sqrt(t(3)) * r
        return var * (one + a) * np.exp(-a), t(3) * r2 / (one + a), -t(1.5) / (one + a), zero
    assert kind == "matern52", kind
    a = np.sqrt(t(5)) * r
    p = one + a + t(5) / t(3) * r * r
    return var * p * np.exp(-a), t(5) / t(3) * r2 * (one + a) / p, -(t(5) / t(6)) * (one + a) / p, zero


def hyper(case, params):
    """exp in double of the stored parameters: what prep_hyper*_kernel leaves in the device's block."""
    g = lambda k: np.exp(np.asarray(params[k], np.float64))
    h = dict(alpha=float(g("log_scale_mixture")) if case["kind"] == "rationalquadratic" else 1.0)
    if case["kind"] == "product":
        h["var"] = float(np.exp(np.float64(params["kern0.log_variance"]) + np.float64(params["kern1.log_variance"])))
    else:
        h["var"] = float(g("log_variance"))
    src = sources(case)
    if src is None:
        h["sc"] = np.broadcast_to(1.0 / g("log_lengthscale"), (case["D"],)).astype(np.float64)
    else:
        h["il"] = [float(np.exp(-np.float64(np.asarray(params[l]).reshape(-1)[0]))) for _, _, l, _ in src]
        h["tp"] = [float(6.283185307179586477 * np.exp(-np.float64(np.asarray(params[p]).reshape(-1)[0]))) if p else 0.0 for _, _, _, p in src]
    return h


def coordinates(case, X, Z, h, t=LD, twice=None):
    """The coordinates the kernels see, in dtype t: (cx (n, D'), cz (M, D'), pert_x, pert_z, pairs).  pert: the relative-to-u perturbation of
    each coordinate the device rounds before the stage (multiply by the unit roundoff of the stored type); pairs: per Periodic axis
    (phase difference t (x - z) (n, M), 1 / ls).  twice: an ARD axis scaled twice (a simulated fault)."""
    X, Z = np.asarray(X, dtype=t), np.asarray(Z, dtype=t)
    src = sources(case)
    if src is None:
        sc = np.asarray(h["sc"], dtype=t).copy()
        if twice is not None:
            sc[twice] = sc[twice] * sc[twice]
        cx, cz = X * sc, Z * sc
        ard = bool(case["opts"].get("ard"))
        # rows: the product x sc_d is rounded; pure_fp32 also rounds the scale of the double block to float32 first (the inducing inputs are
        # scaled in double and rounded once)
        px = np.abs(cx).astype(np.float64) * ((2.0 if case["ctx"] == "pure" else 1.0) if ard else 0.0)
        pz = np.abs(cz).astype(np.float64) * (1.0 if ard else 0.0)
        return cx, cz, px, pz, []
    npair = sum(1 for s in src if s[1])
    Dp = 2 * npair + len(src) - npair
    cx, cz = np.zeros((X.shape[0], Dp), dtype=t), np.zeros((Z.shape[0], Dp), dtype=t)
    px, pz = np.zeros(cx.shape), np.zeros(cz.shape)
    pairs = []
    for j, (ax, pair, _, _) in enumerate(src):
        il, tp = t(h["il"][j]), t(h["tp"][j])
        if pair:
            for c, x, p in ((cx, X, px), (cz, Z, pz)):
                c[:, 2 * j], c[:, 2 * j + 1] = np.cos(tp * x[:, ax]) * il, np.sin(tp * x[:, ax]) * il
                p[:, 2 * j] = p[:, 2 * j + 1] = (np.abs(tp * x[:, ax]).astype(np.float64) + 3.0) * float(il)
            pairs.append((tp * (X[:, ax, None] - Z[None, :, ax]), il))
        else:
            cx[:, npair + j], cz[:, npair + j] = X[:, ax] * il, Z[:, ax] * il
            px[:, npair + j], pz[:, npair + j] = np.abs(cx[:, npair + j]).astype(np.float64), np.abs(cz[:, npair + j]).astype(np.float64)
    return cx, cz, px, pz, pairs


def knm(case, X, Z, params, t=LD, root_eps=True, twice=None):
    """The reference K_nm and everything the backward's terms need, in dtype t, with the bound of K_nm (float64).
    X, Z, params: as stored on the device, cast up.  Returns a dict: k, r2, fl, fr, fa (the three factors), dd (list of the D' coordinate
    differences x_d - z_d (n, M)), pairs, bound, dr2_in (the input perturbation of r2, in units of u)."""
    h = hyper(case, params)
    cx, cz, px, pz, pairs = coordinates(case, X, Z, h, t, twice)
    src = sources(case)
    if src is None:             # the direct form: the difference of the stored coordinates first (no cancellation of the scaled ones), then the scale
        sc = np.asarray(h["sc"], dtype=t).copy()
        if twice is not None:
            sc[twice] = sc[twice] * sc[twice]
        Xt, Zt = np.asarray(X, dtype=t), np.asarray(Z, dtype=t)
        dd = [(Xt[:, d, None] - Zt[None, :, d]) * sc[d] for d in range(cx.shape[1])]
    else:
        dd = [cx[:, d, None] - cz[None, :, d] for d in range(cx.shape[1])]
        for j, (ax, pair, _, _) in enumerate(src):
            if not pair:
                Xt, Zt = np.asarray(X, dtype=t), np.asarray(Z, dtype=t)
                dd[len(pairs) + j] = (Xt[:, ax, None] - Zt[None, :, ax]) * t(h["il"][j])
    if src is None:
        r2 = sum(e * e for e in dd)
    else:                       # the closed formula: 4 sin^2(t (x - z) / 2) / ls^2 per Periodic axis, (x - z)^2 / ls^2 per RBF axis
        npair = len(pairs)
        r2 = sum(t(4) * np.sin(ph / t(2)) ** 2 * il * il for ph, il in pairs) + sum(dd[2 * npair + j] ** 2 for j in range(len(dd) - 2 * npair))
    k, fl, fr, fa = profile(case["kind"], r2, h["var"], h["alpha"], t, root_eps)
    # the isotropic kernels' G is in the RAW coordinates (the device scales r2, not the rows); ARD and periodic contexts keep the scaled ones
    raw = src is None and not case["opts"].get("ard")
    out = dict(k=k, r2=r2, fl=fl, fr=fr, fa=fa, dd=dd, pairs=pairs, h=h, g_unscale=(t(1) / t(h["sc"][0])) if raw else t(1))
    # ---- the bound
    f = facts(case)
    u = U32 if case["ctx"] == "pure" else U64
    D = f["D"]
    k64, r264, fr64 = np.abs(k).astype(np.float64), r2.astype(np.float64), np.abs(fr).astype(np.float64)
    add = [np.abs(e).astype(np.float64) for e in dd]
    dr2_in = sum(2.0 * add[d] * (px[:, d, None] + pz[None, :, d]) for d in range(len(dd)))       # times u
    out["dr2_in"] = dr2_in
    hyp_k, hyp_r2 = 2.0 * U64 + (u if case["ctx"] == "pure" else 0.0), 6.0 * U64 + (u if case["ctx"] == "pure" else 0.0)
    if f["rbf_f64"]:
        c = math.sqrt(0.5 * 1.4426950408889634)                 # the kernel's coordinates: a x = c * (x / ls)
        ax = sum(add[d] * (np.abs(cx[:, d, None]).astype(np.float64) + np.abs(cz[None, :, d]).astype(np.float64)) for d in range(len(dd)))
        tq = c * c * r264                                       # sum dd^2 in the kernel's coordinates
        lv = abs(math.log2(h["var"]))
        err_t = u * (2.0 * c * c * ax + 6.0 * tq + D * (lv + tq) + lv) + u * c * c * dr2_in
        out["bound"] = k64 * (math.log(2.0) * err_t + POLY_REMAINDER + 4.0 * u + hyp_k + hyp_r2 * 0.5 * r264)
    else:
        kind = case["kind"]
        if kind == "matern52":
            prof = 8.0
        elif kind == "rationalquadratic":
            with np.errstate(divide="ignore"):
                prof = np.maximum(4.0, 2.0 + h["alpha"] + 2.0 * np.abs(np.log(np.maximum(k64, 1e-300) / h["var"])))
        else:
            prof = 4.0
        out["bound"] = k64 * (((D + 2 + C_ARG[kind]) * u + hyp_r2) * r264 * fr64 + prof * u + hyp_k) + k64 * fr64 * dr2_in * u
    if case["ctx"] == "pure":
        out["bound"] = out["bound"] + TINY32
    return out


def knm_decimal(case, X, Z, params, pairs_nj, digits=50):
    """k(x_n, z_j) at the given (n, j) pairs with `digits` decimal digits (the standard library's decimal: exp, ln and sqrt; sin by its
    series), from the same stored inputs and the same float64 hyper-parameters as knm().  What the long-double reference is itself checked
    against: a float64 evaluation cannot be (its own rounding is what the bounds of the f64 solve measure)."""
    import decimal
    Dc = decimal.Decimal
    with decimal.localcontext() as cx:
        cx.prec = digits
        h = hyper(case, params)
        var, al = Dc(h["var"]), Dc(h["alpha"])
        pi = Dc("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")

        def sin(x):
            x = x - 2 * pi * (x / (2 * pi)).to_integral_value()
            term, tot, i = x, x, 1
            while abs(term) > Dc(10) ** (-digits - 5):
                term = -term * x * x / ((i + 1) * (i + 2))
                tot, i = tot + term, i + 2
            return tot
        out = []
        src = sources(case)
        for n, j in pairs_nj:
            x, z = [Dc(float(v)) for v in X[n]], [Dc(float(v)) for v in Z[j]]
            if src is None:
                r2 = sum(((a - b) * Dc(float(sc))) ** 2 for a, b, sc in zip(x, z, h["sc"]))
            else:
                r2 = Dc(0)
                for i, (ax, pair, _, _) in enumerate(src):
                    il, d = Dc(h["il"][i]), x[ax] - z[ax]
                    r2 += 4 * sin(Dc(h["tp"][i]) * d / 2) ** 2 * il * il if pair else (d * il) ** 2
            kind = case["kind"]
            if kind in ("rbf", "periodic", "product"):
                k = var * (-r2 / 2).exp()
            elif kind == "rationalquadratic":
                k = var * (-al * (1 + r2 / (2 * al)).ln()).exp()
            else:
                r = (r2 + Dc(1e-12)).sqrt()
                if kind == "exponential":
                    k = var * (-r).exp()
                elif kind == "matern32":
                    a = Dc(3).sqrt() * r
                    k = var * (1 + a) * (-a).exp()
                else:
                    a = Dc(5).sqrt() * r
                    k = var * (1 + a + Dc(5) / Dc(3) * r * r) * (-a).exp()
            out.append(k)
        return out


# ---- W, q, the backward sums, G^T --------------------------------------------------------------------------------------------------------

def _mm(a, b, t):
    return np.asarray(a, dtype=t) @ np.asarray(b, dtype=t)


def _abs_mm(a, b):
    return np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64))


def w_ref(case, Knm, Linv, t=LD, ranges=None):
    """W = K_nm L^-T and its elementwise bound.  ranges: {column tile: (kb, ke)} overriding the reduction range of a tile (simulated faults)."""
    f = facts(case)
    W = _mm(Knm, np.asarray(Linv).T, t)
    for ct, (kb, ke) in (ranges or {}).items():
        cols = slice(ct * f["cw"], min((ct + 1) * f["cw"], case["M"]))
        W[:, cols] = _mm(np.asarray(Knm)[:, kb:ke], np.asarray(Linv)[cols, kb:ke].T, t)
    u = U32 if case["ctx"] == "pure" else U64
    u_store = U32 if case["ctx"] == "f32" else 0.0
    bound = gamma(f["Mp"], u) * _abs_mm(Knm, np.asarray(Linv).T) + u_store * np.abs(W).astype(np.float64)
    if case["ctx"] == "pure":
        bound = bound + (f["Mp"] + 1) * TINY32
    return W, bound


def q_ref(case, W_stored, W_exact=None, W_bound=None, t=LD):
    """q_n = sum_j W[n][j]^2 from the stored W with its bound; with W_exact and W_bound also the reference and bound against the unrounded
    product.  The device adds the squares of its accumulators in the solve precision, stores one partial per column tile in the array
    type and adds those in the array type: gamma(Mp) in the coarser of the two types, plus two roundoffs of the stored W."""
    f = facts(case)
    u_q = U64 if case["ctx"] == "f64" else U32
    u_store = U32 if case["ctx"] == "f32" else 0.0
    Ws = np.asarray(W_stored, dtype=t)
    q = (Ws * Ws).sum(1)
    b1 = (gamma(f["Mp"], u_q) + 2.0 * u_store) * q.astype(np.float64) + ((f["Mp"] + 1) * TINY32 if case["ctx"] == "pure" else 0.0)
    if W_exact is None:
        return q, b1
    We = np.asarray(W_exact, dtype=t)
    q2 = (We * We).sum(1)
    b2 = gamma(f["Mp"], u_q) * q2.astype(np.float64) + 2.0 * (np.abs(We).astype(np.float64) * W_bound).sum(1)
    b2 = b2 + ((f["Mp"] + 1) * TINY32 if case["ctx"] == "pure" else 0.0)
    return q, b1, q2, b2


def terms(case, kn, Knm_got, t=LD):
    """The factor of Kbar in every sum of the backward, from the STORED K_nm (as the device does) and the reference's factors:
    {"s1", "s2", "s3": (n, M); "G": (D', n, M); "axis": (D', n, M); "period": (npair, n, M)} and, per entry, the input-perturbation factor
    (in units of u) as the second dict."""
    kv = np.asarray(Knm_got, dtype=t)
    w = kv * kn["fr"]
    two = t(2)
    T = dict(s1=kv, s2=kv * kn["fl"], s3=kv * kn["fa"], G=np.stack([-w * e * kn["g_unscale"] for e in kn["dd"]]), axis=np.stack([-two * w * e * e for e in kn["dd"]]))
    if kn["pairs"]:
        T["period"] = np.stack([-two * w * ph * np.sin(ph) * il * il for ph, il in kn["pairs"]])
    # input perturbation (ARD, periodic): through r2 for the r2-dependent factors, through the difference itself for G and the axis sums
    r264, dr2 = kn["r2"].astype(np.float64), kn["dr2_in"]
    rel = np.divide(dr2, r264, out=np.zeros_like(dr2), where=r264 > 0)
    P = dict(s1=np.zeros_like(rel), s2=np.abs(T["s2"]).astype(np.float64) * rel, s3=np.abs(T["s3"]).astype(np.float64) * rel)
    P["G"] = np.abs(T["G"]).astype(np.float64) * rel
    P["axis"] = np.abs(T["axis"]).astype(np.float64) * 3.0 * rel
    if "period" in T:
        P["period"] = np.abs(T["period"]).astype(np.float64) * 3.0 * rel
    return T, P


def kbar_ref(case, Wbar, Linv, t=LD, ranges=None):
    """Kbar = Wbar L^-1 and its elementwise bound (the f64 solve accumulates the float32 Wbar exactly cast up)."""
    f = facts(case)
    Kb = _mm(Wbar, Linv, t)
    for ct, (kb, ke) in (ranges or {}).items():
        cols = slice(ct * f["cw"], min((ct + 1) * f["cw"], case["M"]))
        Kb[:, cols] = _mm(np.asarray(Wbar)[:, kb:ke], np.asarray(Linv)[kb:ke, cols], t)
    u = U32 if case["ctx"] == "pure" else U64
    return Kb, gamma(f["Mp"], u) * _abs_mm(Wbar, Linv) + ((f["Mp"] + 1) * TINY32 if case["ctx"] == "pure" else 0.0)


def sums(case, Kb, Kb_bound, T, P, rows=None):
    """Every sum of the backward with its bound: {"s1", "s2", "s3": scalar; "G": (M, D'); "axis": (D',); "period": (npair,)} twice (value, bound).
    rows: a weight per row (simulated faults: a row dropped or counted twice)."""
    u = U32 if case["ctx"] == "pure" else U64
    g = gamma(SUM_TERMS, u) + c_term(facts(case)["D"]) * u
    w = np.ones(Kb.shape[0]) if rows is None else np.asarray(rows, np.float64)
    Kw = Kb * np.asarray(w, dtype=Kb.dtype)[:, None]
    aK, bK = np.abs(Kw).astype(np.float64), Kb_bound * np.abs(w)[:, None]
    val, bnd = {}, {}
    for name, tm in T.items():
        per_col = name == "G"
        axes = (-2,) if per_col else (-2, -1)
        val[name] = (Kw * tm).sum(axis=axes)
        at = np.abs(tm).astype(np.float64)
        bnd[name] = (bK * at + g * aK * at + u * aK * P[name] + (TINY32 if case["ctx"] == "pure" else 0.0)).sum(axis=axes)
        if per_col:
            val[name], bnd[name] = val[name].T, bnd[name].T          # (M, D')
    return val, bnd


def tn_bounds(case, Wbar, W_stored, W_bound, T, Linv):
    """hyper_backward="tn": the bounds of red_d[4] = sum Wbar W (double accumulation of the stored operands) and of red_d[5] through
    Hd = dK^T Wbar on the split fp16 kernel, contracted with L^-1 in double."""
    aWb = np.abs(np.asarray(Wbar, np.float64))
    n_terms = aWb.size
    b4 = (aWb * W_bound).sum() + gamma(n_terms, U64) * (aWb * np.abs(np.asarray(W_stored, np.float64))).sum()
    Hd = np.asarray(T["s2"], np.float64).T @ np.asarray(Wbar, np.float64)
    aL = np.abs(np.tril(np.asarray(Linv, np.float64))).sum()
    b5 = SPLIT_TOL * np.abs(Hd).max() * aL + gamma(case["M"], U64) * (np.abs(Hd) * np.abs(np.asarray(Linv, np.float64)).T).sum()
    return b4, b5


def gt_ref(case, W_stored, Wbar, t=LD):
    G = _mm(np.asarray(W_stored).T, Wbar, t)
    u = U64 if case["ctx"] == "f64" else U32
    bound = gamma(case["n"], u) * _abs_mm(np.asarray(W_stored).T, Wbar)
    if case["ctx"] != "f64":
        bound = bound + SPLIT_TOL * float(np.abs(G).max()) + case["n"] * TINY32
    return G, bound


# ---- measures ---------------------------------------------------------------------------------------------------------------------------

def ratio(got, ref, bound):
    """max |got - ref| / bound, the difference formed in long double; infinity where got is not finite or a zero bound is exceeded."""
    got, ref, bound = np.asarray(got), np.asarray(ref, dtype=LD), np.asarray(bound, np.float64)
    if not np.isfinite(np.asarray(got, np.float64)).all():
        return float("inf")
    e = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    r = np.where(bound > 0, e / np.where(bound > 0, bound, 1.0), np.where(e > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def tile_ratio(got, ref, bound, rt=TILE, ct=64):
    """max over the rt x ct tiles of  max |got - ref| / max bound  inside the tile (in the style of test_gpu_topic_forms._tile_err): a tile
    that is wrong as a whole shows even where its largest elements hide the others."""
    got, ref, bound = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bound, np.float64)
    R, Cn = ref.shape
    nr, nc = -(-R // rt), -(-Cn // ct)
    pad = [(0, nr * rt - R), (0, nc * ct - Cn)]
    e = np.pad(np.abs(got - ref).astype(np.float64), pad).reshape(nr, rt, nc, ct).max(axis=(1, 3))
    b = np.pad(bound, pad).reshape(nr, rt, nc, ct).max(axis=(1, 3))
    return float(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e > 0, np.inf, 0.0)).max())


def tile_shares(case, A):
    """Per (128-row tile, column tile of the solve type) the share of sum |A| (n, M) the tile carries."""
    f = facts(case)
    A = np.abs(np.asarray(A, np.float64))
    R, Cn = A.shape
    nr, nc = -(-R // TILE), -(-Cn // f["cw"])
    s = np.pad(A, [(0, nr * TILE - R), (0, nc * f["cw"] - Cn)]).reshape(nr, TILE, nc, f["cw"]).sum(axis=(1, 3))
    return s / s.sum()


def tile_max(case, A):
    f = facts(case)
    A = np.abs(np.asarray(A, np.float64))
    R, Cn = A.shape
    nr, nc = -(-R // TILE), -(-Cn // f["cw"])
    m = np.pad(A, [(0, nr * TILE - R), (0, nc * f["cw"] - Cn)]).reshape(nr, TILE, nc, f["cw"]).max(axis=(1, 3))
    return m / m.max()


def no_negligible_tile(case, W, Kb, T):
    """The smallest share any (row tile, column tile) carries of max |W| and of sum |Kbar dK| of each scalar sum (s3: RationalQuadratic only)."""
    out = dict(W=float(tile_max(case, W).min()))
    for name in ("s1", "s2") + (("s3",) if case["kind"] == "rationalquadratic" else ()):
        out[name] = float(tile_shares(case, np.asarray(Kb, np.float64) * np.asarray(T[name], np.float64)).min())
    return out


# ---- the host's stand-ins for what the device supplies ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host_operands(name):
    """K_nm, L^-1 and a W-bar for the CPU tests: the reference K_nm rounded to the solve precision, numpy's Cholesky factor of
    K_uu + jitter I in the solve precision and its inverse, and a random W-bar shaped like the device's (a term locbar^T U and a dense one) whose last, ragged row tile is 20x as
    large (as the counts make the device's).  Read-only."""
    case = CASES[name]
    d = inputs(name)
    st = stored(d, case)
    ts = solve_dtype(case)
    kn = knm(case, st["X"], st["Z"], st["params"])
    Knm = kn["k"].astype(ts).astype(np.float64)
    kuu = knm(case, st["Z"], st["Z"], st["params"])["k"].astype(ts)
    L = np.linalg.cholesky(kuu + ts(JITTER_TOTAL) * np.eye(case["M"], dtype=ts))           # raises LinAlgError if not positive definite
    assert L.dtype == ts
    Linv = np.tril(np.linalg.inv(L.astype(np.float64))).astype(ts).astype(np.float64)
    rng = np.random.default_rng(case["M"] + case["n"])
    Wbar = rng.standard_normal((case["n"], case["K"])) @ np.asarray(st["params"]["u_loc"]) + 0.3 * rng.standard_normal((case["n"], case["M"]))
    Wbar[(case["n"] - 1) // TILE * TILE:] *= 20
    Wbar = Wbar.astype(array_dtype(case)).astype(np.float64)
    for a in (Knm, Linv, Wbar):
        a.setflags(write=False)
    return dict(case=case, st=st, kn=kn, Knm=Knm, Linv=Linv, Wbar=Wbar)
