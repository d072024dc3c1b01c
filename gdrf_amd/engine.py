"""Host-side driver of libgdrf_hip: owns the device context, the flat unconstrained-parameter /
gradient / optimizer-state buffers (PyTorch-ROCm tensors used as storage only) and sequences one
SVI step:  factorize (jitter retry) -> step_local -> [RCCL all-reduce] -> step_finish -> adam.

Reference behaviour mirrored here (paths under /root/reference):
  jittercholesky retry schedule        gdrf/models/utils.py:27-40
  SVI.step / 1/N scaling               gdrf/train_script.py:365-371,467
  parameter initialisation             gdrf/models/sparse_gdrf.py:96-122, abstract_gdrf.py:57-84
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .data import check_counts, is_sparse_counts

KERNEL_IDS = {"rbf": 0, "matern52": 1, "matern32": 2, "exponential": 3, "rationalquadratic": 4, "periodic": 5, "product": 6}
# factor kinds of a product context's table (gdrf_set_product)
PRODUCT_KINDS = {"rbf": 0, "periodic": 5}
OPT_MODES = {"adam": 0, "adamw": 1, "clippedadam": 2}
# update rules of gdrf_optim_step (include/gdrf_hip.h)
OPT_RULES = {"adam": 0, "adamw": 1, "clippedadam": 2, "adamax": 3, "rmsprop": 4, "adagrad": 5, "adadelta": 6, "asgd": 7, "rprop": 8,
             "adagradrmsprop": 9}
OPT_CLIP_NORM, OPT_CLIP_VALUE, OPT_MOMENTUM, OPT_CENTERED = 1, 2, 4, 8

_WS_IDS = dict(W=0, Wbar=1, q=2, loc=3, tt=4, vbar=5, locbar=6, asum=7, Kuu=8, L=9, Linv=10, S=11, B=12, phi=13,
               mu=14, LinvT=15, ST=16, Knm=17, g_locbar=18)


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def check_mc_args(num_samples, K: int, n: int, eps=None, ws=None) -> int:
    """The argument errors of the Monte-Carlo predictive calls (Engine.predict_mc and the model methods above it), raised before the
    device is touched: ``num_samples`` >= 1, an injected ``eps`` of shape (num_samples, K, n), dense counts.  Returns num_samples as an int."""
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    if eps is not None and tuple(eps.shape) != (S, K, n):
        raise ValueError(f"eps must have shape (num_samples, K, n) = ({S}, {K}, {n}), got {tuple(eps.shape)}")
    if ws is not None and is_sparse_counts(ws):
        raise ValueError("the Monte-Carlo predictive score reads dense counts: a sparse (CSR) ws is not supported")
    return S


def check_fold_args(num_iters, tol, n: int, V: int, ws, ws_score=None):
    """The argument errors of the fold-in calls (Engine.fold_in and the model methods above it), raised before the device is touched: an
    integral ``num_iters`` >= 0, a finite ``tol`` >= 0, counts ``ws`` of shape (n, V) with n >= 1, dense or CSR, and a ``ws_score`` of the
    same shape and sparsity.  Returns (num_iters, tol) as an int and a float."""
    if isinstance(num_iters, bool) or int(num_iters) != num_iters:
        raise ValueError(f"num_iters must be an integer, got {num_iters!r}")
    if int(num_iters) < 0:
        raise ValueError(f"num_iters must be >= 0, got {num_iters}")
    tol = float(tol)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"tol must be finite and >= 0, got {tol}")
    if n < 1:
        raise ValueError(f"fold-in needs at least one row, got {n}")
    for name, w in (("ws", ws), ("ws_score", ws_score)):
        if w is None and name == "ws_score":
            continue
        if w is None or not hasattr(w, "shape") or tuple(w.shape) != (n, V):
            raise ValueError(f"{name} must be counts of shape (n, V) = ({n}, {V}), got {None if w is None else tuple(getattr(w, 'shape', ()))}")
    if ws_score is not None and is_sparse_counts(ws_score) != is_sparse_counts(ws):
        raise ValueError("ws_score must be sparse (CSR) exactly when ws is: the scored counts take the layout of the fitted ones")
    return int(num_iters), tol


# The rows of Engine.predict_info's (6, n) result, in order, and the words of Phi its kernel stages in LDS at a time (GDRF_INFO_V_CHUNK of
# include/gdrf_hip.h): a larger V is served chunk by chunk.
INFO_NAMES = ("topic_entropy", "topic_expected_entropy", "topic_information", "word_entropy", "word_expected_entropy", "word_information")
INFO_V_CHUNK = 128

# The rows of Engine.predict_score's (5, n) result, in order, the words of Phi its dense form stages in LDS at a time and the samples whose
# log likelihoods a row keeps there while the chunks pass (GDRF_SCORE_V_CHUNK and GDRF_SCORE_S_TILE of include/gdrf_hip.h): neither limits
# V or num_samples.
SCORE_NAMES = ("lpd", "mean_log_lik", "var_log_lik", "total", "log_coef")
SCORE_V_CHUNK = 128
SCORE_S_TILE = 64


def check_score_args(num_samples, K: int, V: int, n: int, ws, eps=None) -> int:
    """The argument errors of the per-row predictive score (Engine.predict_score and the model methods above it), raised before the device
    is touched: an integral ``num_samples`` in 1 .. 65535, an injected ``eps`` of shape (num_samples, K, n), counts ``ws`` of shape
    (n, V) with n >= 1, dense or CSR.  Returns num_samples as an int."""
    try:
        integral = not isinstance(num_samples, bool) and int(num_samples) == num_samples
    except (TypeError, ValueError, OverflowError):
        integral = False
    if not integral:
        raise ValueError(f"num_samples must be an integer, got {num_samples!r}")
    S = int(num_samples)
    if not 1 <= S <= 65535:
        raise ValueError(f"num_samples must be in 1 .. 65535, got {S}")
    if n < 1:
        raise ValueError(f"the predictive score needs at least one row, got {n}")
    if eps is not None and (not hasattr(eps, "shape") or tuple(eps.shape) != (S, K, n)):
        raise ValueError(f"eps must have shape (num_samples, K, n) = ({S}, {K}, {n}), got {tuple(getattr(eps, 'shape', ()))}")
    if ws is None or not hasattr(ws, "shape") or tuple(ws.shape) != (n, V):
        raise ValueError(f"ws must be counts of shape (n, V) = ({n}, {V}), got {None if ws is None else tuple(getattr(ws, 'shape', ()))}")
    return S


# The rows of Engine.predict_loo's (6, n) result, in order (Engine.psis_rows returns the first three), and the range of num_samples: all of
# a row's log likelihoods are kept and ordered in LDS, and a tail of fewer than five values is not fitted (GDRF_LOO_* of
# include/gdrf_hip.h).
LOO_NAMES = ("elpd_loo", "pareto_k", "ess", "lpd", "total", "log_coef")
LOO_MAX_SAMPLES = 1024
LOO_MIN_SAMPLES = 25


def loo_tail_len(num_samples: int) -> int:
    """M = ceil(min(S / 5, 3 sqrt(S))): the largest importance ratios of a row that PSIS fits the generalised Pareto tail to, in double
    as the library forms it (csrc/forms.h::loo_tail_len)."""
    S = int(num_samples)
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S))))


def _loo_samples(num_samples) -> int:
    try:
        integral = not isinstance(num_samples, bool) and int(num_samples) == num_samples
    except (TypeError, ValueError, OverflowError):
        integral = False
    if not integral:
        raise ValueError(f"num_samples must be an integer, got {num_samples!r}")
    S = int(num_samples)
    if not LOO_MIN_SAMPLES <= S <= LOO_MAX_SAMPLES:
        raise ValueError(f"num_samples must be in {LOO_MIN_SAMPLES} .. {LOO_MAX_SAMPLES}, got {S}")
    return S


def check_loo_args(num_samples, K: int, V: int, n: int, ws, eps=None) -> int:
    """The argument errors of PSIS leave-one-out (Engine.predict_loo and the model methods above it), raised before the device is
    touched: those of check_score_args with ``num_samples`` in LOO_MIN_SAMPLES .. LOO_MAX_SAMPLES.  Returns num_samples as an int."""
    return check_score_args(_loo_samples(num_samples), K, V, n, ws, eps)


def check_psis_args(log_lik) -> Tuple[int, int]:
    """The argument errors of the PSIS stage on a caller's own matrix (Engine.psis_rows, the model's psis): a (S, n) tensor with S in
    LOO_MIN_SAMPLES .. LOO_MAX_SAMPLES and n >= 1.  Returns (S, n)."""
    if not torch.is_tensor(log_lik) or log_lik.dim() != 2 or log_lik.shape[1] < 1:
        raise ValueError(f"log_lik must be a (num_samples, n) tensor with n >= 1, got {tuple(getattr(log_lik, 'shape', ()))}")
    return _loo_samples(int(log_lik.shape[0])), int(log_lik.shape[1])


# Engine.predict_quant (gdrf_predict_quant, csrc/predict_quant.h): its modes, the most samples the quantile mode orders in LDS and the most
# levels (quantile levels or thresholds) of a call - GDRF_QUANT_* of include/gdrf_hip.h.  The counter modes take the 65535 samples of
# their siblings.
QUANT_QUANTILE, QUANT_EXCEED, QUANT_DOMINANT = 0, 1, 2
QUANT_MAX_SAMPLES = 1024
QUANT_MAX_LEVELS = 16


def check_quant_args(mode, num_samples, K: int, V: int, n: int, levels=None, words=None, eps=None):
    """The argument errors of the quantile, exceedance and dominant-topic calls (Engine.predict_quant and the model methods above it),
    raised before the device is touched: a known ``mode``; ``num_samples`` >= 1, at most QUANT_MAX_SAMPLES for quantiles and 65535
    otherwise; an injected ``eps`` of shape (num_samples, K, n); 1 .. QUANT_MAX_LEVELS ``levels`` - quantile levels in [0, 1] or finite
    thresholds, a scalar counts as one -, none for the dominant-topic mode; ``words`` a non-empty 1-D list of integers in [0, V), none for
    the dominant-topic mode.  The word list is validated here and nowhere below: the library reads it on the device only.
    Returns (num_samples, levels as a list of floats, number of words or 0)."""
    if isinstance(mode, bool) or mode not in (QUANT_QUANTILE, QUANT_EXCEED, QUANT_DOMINANT):
        raise ValueError(f"predict_quant: mode must be 0 (quantiles), 1 (exceedance) or 2 (dominant topic), got {mode!r}")
    S = check_mc_args(num_samples, K, n, eps)
    cap = QUANT_MAX_SAMPLES if mode == QUANT_QUANTILE else 65535
    if S > cap:
        raise ValueError(f"num_samples must be <= {cap} for this mode, got {S}")
    lv = []
    if mode == QUANT_DOMINANT:
        if levels is not None:
            raise ValueError("the dominant-topic mode takes no levels")
        if words is not None:
            raise ValueError("the dominant-topic mode is over topics: it takes no words")
    else:
        what = "quantile level" if mode == QUANT_QUANTILE else "threshold"
        lv = [] if levels is None else [float(v) for v in torch.as_tensor(levels, dtype=torch.float64).reshape(-1)]
        if not 1 <= len(lv) <= QUANT_MAX_LEVELS:
            raise ValueError(f"needs between 1 and QUANT_MAX_LEVELS = {QUANT_MAX_LEVELS} {what}s, got {len(lv)}")
        for v in lv:
            if mode == QUANT_QUANTILE and not 0.0 <= v <= 1.0:
                raise ValueError(f"a quantile level must be in [0, 1], got {v}")
            if mode == QUANT_EXCEED and not math.isfinite(v):
                raise ValueError(f"a threshold must be finite, got {v}")
    nw = 0
    if words is not None:
        w = torch.as_tensor(words)
        if w.dim() != 1 or w.numel() < 1 or w.dtype.is_floating_point or w.dtype.is_complex or w.dtype == torch.bool:
            raise ValueError(f"words must be a non-empty 1-D list of integer word indices, got shape {tuple(w.shape)} of {w.dtype}")
        lo, hi = int(w.min()), int(w.max())
        if lo < 0 or hi >= V:
            raise ValueError(f"every word index must be in [0, V = {V}), got {lo if lo < 0 else hi}")
        nw = int(w.numel())
    return S, lv, nw


# The most words (V) the count sampler serves (GDRF_SC_MAX_V of include/gdrf_hip.h): a wave keeps a row's CDF, counts and p in LDS.
SAMPLE_COUNTS_MAX_V = 4096


def check_count_args(theta, totals, K: int, V: int, mode: int = 0, ws=None, u=None, row_offset=0):
    """The argument errors of the count sampler (Engine.sample_counts and the model methods above it), raised before the device is
    touched: V <= SAMPLE_COUNTS_MAX_V, ``theta`` of shape (S, n, K) with S, n >= 1, ``totals`` (n,) integers >= 0, ``row_offset`` >= 0,
    for mode 1 dense counts ``ws`` of shape (n, V), an injected ``u`` of shape (S, n, >= max totals) float64 with every entry in [0, 1).
    Returns (S, n, tmax)."""
    if V > SAMPLE_COUNTS_MAX_V:
        raise ValueError(f"sample_counts serves at most SAMPLE_COUNTS_MAX_V = {SAMPLE_COUNTS_MAX_V} observation categories, the model has {V}")
    if mode not in (0, 1):
        raise ValueError("sample_counts: mode must be 0 (replicated counts) or 1 (predictive-check statistics)")
    if theta is None or not hasattr(theta, "shape") or len(theta.shape) != 3 or theta.shape[2] != K or theta.shape[0] < 1 or theta.shape[1] < 1:
        raise ValueError(f"theta must have shape (num_samples, n, K = {K}) with num_samples, n >= 1, "
                         f"got {None if theta is None else tuple(getattr(theta, 'shape', ()))}")
    S, n = int(theta.shape[0]), int(theta.shape[1])
    if S > 65535:
        raise ValueError(f"sample_counts takes at most 65535 samples in one call, got {S}")
    if not torch.is_tensor(totals) or tuple(totals.shape) != (n,):
        raise ValueError(f"totals must be a tensor of shape (n,) = ({n},), got {tuple(getattr(totals, 'shape', ()))}")
    if totals.dtype.is_floating_point or totals.dtype.is_complex or totals.dtype == torch.bool:
        raise ValueError(f"totals must be integers, got {totals.dtype}")
    tmin, tmax = int(totals.min()), int(totals.max())
    if tmin < 0:
        raise ValueError(f"totals must be >= 0, got {tmin}")
    if tmax > 2 ** 31 - 4:
        raise ValueError(f"totals must fit an int32, got {tmax}")
    if int(row_offset) < 0:
        raise ValueError(f"row_offset must be >= 0, got {row_offset}")
    if ws is not None and is_sparse_counts(ws):
        raise ValueError("the predictive check reads dense counts: a sparse (CSR) ws is not supported")
    if mode == 1 and (ws is None or not hasattr(ws, "shape") or tuple(ws.shape) != (n, V)):
        raise ValueError(f"mode 1 needs the observed counts ws of shape (n, V) = ({n}, {V}), got {None if ws is None else tuple(getattr(ws, 'shape', ()))}")
    if mode == 0 and ws is not None:
        raise ValueError("sample_counts: ws is read by mode 1 only")
    if u is not None:
        if not torch.is_tensor(u) or u.dim() != 3 or tuple(u.shape[:2]) != (S, n) or u.dtype != torch.float64:
            raise ValueError(f"u must be a float64 tensor of shape (num_samples, n, tmax) = ({S}, {n}, >= {tmax}), "
                             f"got {getattr(u, 'dtype', None)} {tuple(getattr(u, 'shape', ()))}")
        if u.shape[2] < tmax:
            raise ValueError(f"u holds {u.shape[2]} tokens per row, the largest total is {tmax}: too few tokens")
        if u.numel() and not bool(((u >= 0.0) & (u < 1.0)).all()):
            raise ValueError("u must lie in [0, 1)")
    return S, n, tmax


# The most rows a joint call (Engine.predict_cov, Engine.sample_joint and the model methods above them) takes: a joint draw cannot be cut
# into row pieces, its n x n factorisation runs in one workgroup and its covariances take K n^2 elements (DESIGN.md section 19 has the
# times and the memory measured at this size).
JOINT_MAX_ROWS = 4096
# the two Philox streams of gdrf_sample_joint (include/gdrf_hip.h): fill_eps(seed, s, n_offset=JOINT_XI_OFFSET, n=M) is xi[s]
JOINT_XI_OFFSET, JOINT_ZETA_OFFSET = 1 << 61, 1 << 62


def check_joint_args(num_samples, K: int, M: int, n: int, xi=None, zeta=None) -> int:
    """The argument errors of the joint calls (Engine.predict_cov, Engine.sample_joint and the model methods above them), raised before
    the device is touched: at most JOINT_MAX_ROWS rows, an integral ``num_samples`` >= 1, an injected ``xi`` of shape (num_samples, K, M)
    and ``zeta`` of shape (num_samples, K, n).  Returns num_samples as an int."""
    if n < 1:
        raise ValueError(f"a joint call needs at least one row, got {n}")
    if n > JOINT_MAX_ROWS:
        raise ValueError(f"a joint call takes all its rows at once and at most JOINT_MAX_ROWS = {JOINT_MAX_ROWS} of them, got {n}")
    if isinstance(num_samples, bool) or int(num_samples) != num_samples:
        raise ValueError(f"num_samples must be an integer, got {num_samples!r}")
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    if xi is not None and tuple(xi.shape) != (S, K, M):
        raise ValueError(f"xi must have shape (num_samples, K, M) = ({S}, {K}, {M}), got {tuple(xi.shape)}")
    if zeta is not None and tuple(zeta.shape) != (S, K, n):
        raise ValueError(f"zeta must have shape (num_samples, K, n) = ({S}, {K}, {n}), got {tuple(zeta.shape)}")
    return S


# The most pivots a batch choice takes (Engine.select_batch): the given rows and the free picks together (GDRF_SELECT_MAX_PICKS of
# include/gdrf_hip.h).  Its factor storage is K x (G + count) x (n + G) solve-precision elements.
SELECT_MAX_PICKS = 256


def check_select_args(count, noise, n: int, given=None, dims: Optional[int] = None):
    """The argument errors of the batch choice (Engine.select_batch and the model method above it), raised before the device is touched:
    an integral ``count`` in [1, n], a ``given`` of shape (G, dims) with G + count <= SELECT_MAX_PICKS, a positive finite ``noise`` (None:
    the caller fills in the model's own and the check is skipped).  Returns (count as an int, noise as a float or None, G)."""
    if n < 1:
        raise ValueError(f"select_batch needs at least one row, got {n}")
    if isinstance(count, bool) or isinstance(count, str) or int(count) != count:
        raise ValueError(f"count must be an integer, got {count!r}")
    cnt = int(count)
    if not 1 <= cnt <= n:
        raise ValueError(f"count must be in [1, N = {n}], got {count}")
    G = 0
    if given is not None:
        shape = tuple(given.shape)
        if len(shape) == 1 and dims == 1:
            shape = (shape[0], 1)
        if len(shape) != 2 or (dims is not None and shape[1] != dims):
            raise ValueError(f"given must have shape (G, {dims}), the columns of xs, got {tuple(given.shape)}")
        G = int(shape[0])
    if G + cnt > SELECT_MAX_PICKS:
        raise ValueError(f"the given rows and the picks together are at most SELECT_MAX_PICKS = {SELECT_MAX_PICKS}, got {G} + {cnt}")
    if noise is not None:
        if isinstance(noise, bool) or not math.isfinite(float(noise)) or not float(noise) > 0.0:
            raise ValueError(f"noise must be a positive finite number, got {noise!r}")
        noise = float(noise)
    return cnt, noise, G


# The most pivots a choice of inducing points takes (Engine.select_inducing): the given rows and the free picks together
# (GDRF_INDUCING_MAX_PICKS of include/gdrf_hip.h).  Its factor storage is (G + count) x (n + G) solve-precision elements, held for the call.
INDUCING_MAX_PICKS = 1024


def check_inducing_args(count, floor, n: int, given=None, dims: Optional[int] = None):
    """The argument errors of the choice of inducing points (Engine.select_inducing and the model method above it), raised before the device
    is touched: an integral ``count`` in [0, n], a ``given`` of shape (G, dims) with 1 <= G + count <= INDUCING_MAX_PICKS, a finite
    ``floor`` >= 0 (None: the caller fills in the model's own and the check is skipped).  Returns (count as an int, floor as a float or
    None, G)."""
    if n < 1:
        raise ValueError(f"select_inducing needs at least one row, got {n}")
    if isinstance(count, bool) or isinstance(count, str) or int(count) != count:
        raise ValueError(f"count must be an integer, got {count!r}")
    cnt = int(count)
    if not 0 <= cnt <= n:
        raise ValueError(f"count must be in [0, N = {n}], got {count}")
    G = 0
    if given is not None:
        shape = tuple(given.shape)
        if len(shape) == 1 and dims == 1:
            shape = (shape[0], 1)
        if len(shape) != 2 or (dims is not None and shape[1] != dims):
            raise ValueError(f"given must have shape (G, {dims}), the columns of xs, got {tuple(given.shape)}")
        G = int(shape[0])
    if G + cnt < 1:
        raise ValueError("count = 0 needs given rows to score: the given rows and the picks together are at least 1")
    if G + cnt > INDUCING_MAX_PICKS:
        raise ValueError(f"the given rows and the picks together are at most INDUCING_MAX_PICKS = {INDUCING_MAX_PICKS}, got {G} + {cnt}")
    if floor is not None:
        if isinstance(floor, bool) or not math.isfinite(float(floor)) or not float(floor) >= 0.0:
            raise ValueError(f"floor must be a finite number >= 0, got {floor!r}")
        floor = float(floor)
    return cnt, floor, G


def thin_rows(n: int, max_candidates: int) -> Optional[torch.Tensor]:
    """The rows a choice among more than ``max_candidates`` rows looks at: floor(i n / c) for i < c = max_candidates, increasing and
    distinct (int64, on the CPU); None when n <= max_candidates: every row."""
    if isinstance(max_candidates, bool) or int(max_candidates) != max_candidates or int(max_candidates) < 1:
        raise ValueError(f"max_candidates must be a positive integer, got {max_candidates!r}")
    c = int(max_candidates)
    if n <= c:
        return None
    return (torch.arange(c, dtype=torch.int64) * n) // c


def param_table(K: int, M: int, V: int, D: int, kernel: str = "rbf", *, ard: bool = False, period_count: int = 0, product=None,
                learn_inducing: bool = False, mean_shapes=None, raw) -> Dict[str, tuple]:
    """{name: (offset, shape)} of every learnt parameter tensor of a context, in the order of Engine.param_names (that of state_dict(),
    parameters() and the optimizer state).  Pure: ``raw`` holds what the library's layout calls returned, {"param": gdrf_param_layout,
    "inducing": gdrf_inducing_layout, "ard": gdrf_ard_layout, "periodic": gdrf_periodic_layout, "product": gdrf_product_layout, "mean":
    gdrf_mean_param_layout}; only the entries the configuration reads have to be there.  ``product`` is the factor table of
    Engine(kernel="product"), ``mean_shapes`` {name: shape} of the mean_function's parameters."""
    lay = raw["param"]
    vec = lambda n: () if n == 1 else (int(n),)
    t: Dict[str, tuple] = {}
    if product is not None:                       # the factors' segments in place of slots 0 and 1
        ov, _, ol, _, op, _ = raw["product"]
        for f, fac in enumerate(product):
            pre = fac["name"] + "." if fac["name"] else ""
            nl, npr = int(fac["lengthscales"]), int(fac.get("periods", 0))
            t[pre + "log_variance"] = (ov + f, ())
            t[pre + "log_lengthscale"] = (ol, vec(nl))
            ol += nl
            if npr:
                t[pre + "log_period"] = (op, vec(npr))
                op += npr
    else:
        t["log_lengthscale"] = (raw["ard"][0], (D,)) if ard else (lay[0], ())
        t["log_variance"] = (lay[1], ())
    t.update(log_noise=(lay[2], ()), u_loc=(lay[3], (K, M)), phi_unc=(lay[4], (K, V)), u_scale_tril_unc=(lay[5], (K, M, M)))
    if kernel == "rationalquadratic":
        t["log_scale_mixture"] = (3, ())
    if period_count:
        t["log_period"] = (raw["periodic"][0], vec(period_count))
    if learn_inducing:
        t["inducing_unc"] = (raw["inducing"][0], (M, D))
    o = raw["mean"][0] if mean_shapes else 0
    for name, shape in (mean_shapes or {}).items():
        t[name] = (o, tuple(shape))
        o += math.prod(shape)
    return t


class Engine:
    """One device context for fixed (n_cap, M, K, V, D, dtype, kernel)."""

    last_joint_jitter: Optional[float] = None    # cumulative jitter on R of the most recent sample_joint, and its level of the schedule
    last_joint_level: Optional[int] = None

    opt_extra: Optional[torch.Tensor] = None     # third optimizer state vector (RMSprop with momentum and centered), on demand

    def __init__(self, n_cap: int, M: int, K: int, V: int, D: int, *, dtype=torch.float32, kernel: str = "rbf",
                 device="cuda:0", jitter: float = 1e-8, maxjitter: int = 15, process_group="auto", pure_fp32: bool = False,
                 store_t="auto", mfma_mode: str = "auto", learn_inducing: bool = False, whiten: bool = True,
                 hyper_backward: str = "auto", allreduce_fn=None, ard: bool = False, mean_params: Optional[Dict[str, tuple]] = None,
                 rows_form: str = "auto", period_count: int = 1, product=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GdrfHipError("gdrf_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GdrfHipError(f"gdrf_amd runs on a HIP device only, got device={device!r}")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        self.dtype = dtype
        self.n_cap, self.M, self.K, self.V, self.D = int(n_cap), int(M), int(K), int(V), int(D)
        self.kernel = kernel
        self.jitter, self.maxjitter = float(jitter), int(maxjitter)
        self.pg = process_group          # "auto": default group when torch.distributed is initialised; None: never reduce
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", dev_index)
        torch.cuda.set_device(dev_index)
        ctx = C.c_void_p()
        _lib.check(self.lib.gdrf_ctx_create_ex(C.byref(ctx), dev_index, self.n_cap, self.M, self.K, self.V, self.D,
                                               (2 if pure_fp32 else 0) if dtype == torch.float32 else 1, KERNEL_IDS[kernel],
                                               {"auto": 2, True: 1, False: 0}[store_t]), "gdrf_ctx_create_ex")
        self.pure_fp32 = bool(pure_fp32) and dtype == torch.float32
        self.ctx = ctx
        self.stores_t = bool(self.lib.gdrf_stores_t(self.ctx))
        # arithmetic of the f32 GEMM-shaped contractions (csrc/gemm_split.h): "f16x3" = two block-scaled fp16 pieces per operand,
        # 3 products; "bf16x6" = three bf16 pieces, 6 products (both: f32 accumulation on the 16-bit matrix path, error held to
        # the native f32 MFMA kernels'); "f32" = native f32 MFMA.  "auto" = f16x3 wherever it applies (float32 arrays with the
        # f64 solve - which bounds |W| by sqrt(variance) -, dense Wbar), bf16x6 for the all-fp32 arithmetic, else f32.
        if mfma_mode not in ("auto", "f32", "bf16x6", "f16x3"):
            raise ValueError("mfma_mode must be 'auto', 'f32', 'bf16x6' or 'f16x3'")
        if mfma_mode == "auto":
            mfma_mode = "f32" if (dtype != torch.float32 or self.stores_t) else ("bf16x6" if self.pure_fp32 else "f16x3")
        self.mfma_mode = mfma_mode
        if mfma_mode != "f32":
            _lib.check(self.lib.gdrf_set_mfma_mode(self.ctx, {"bf16x6": 1, "f16x3": 2}[mfma_mode]), "gdrf_set_mfma_mode")
        # K_nm parts of the kernel hyper-parameter gradients: "f64" (= "auto") = Kbar = Wbar L^-1 on the f64 matrix pipe; "tn" = Hd = dK^T Wbar
        # on the split TN kernel + an M x M contraction with L^-1 in double (csrc/hyper_tn.h; no f64 backward GEMM: faster, but d / d log
        # lengthscale then carries float32-level rounding through the cancelling contraction: 3.6e-4 instead of 1e-7 at the headline grid)
        if hyper_backward not in ("auto", "tn", "f64"):
            raise ValueError("hyper_backward must be 'auto', 'tn' or 'f64'")
        _lib.check(self.lib.gdrf_set_hyper_backward(self.ctx, 1 if hyper_backward == "tn" else 0), "gdrf_set_hyper_backward")
        self._hyper_backward_request = hyper_backward
        # the per-row terms that touch the vocabulary (gdrf_set_rows_form): "auto" = the LDS row forms (Phi and its gradient in LDS; K x V
        # bounded, larger shapes fail with "too large"); "streamed" = Phi through LDS in tiles of words, any V and K <= 128 (csrc/rows_vstream.h).
        # "auto" governs the ordinary step and predict; a custom link_function and the two-point step (xs_guide) are streamed in either setting
        if rows_form not in ("auto", "streamed"):
            raise ValueError("rows_form must be 'auto' or 'streamed'")
        if rows_form == "streamed":
            _lib.check(self.lib.gdrf_set_rows_form(self.ctx, 1), "gdrf_set_rows_form")
        # a caller-owned collective behind the C ABI (gdrf_set_allreduce): fn(buf_ptr, count, is_double, stream_ptr) -> 0 sums the flat payload in
        # place over the caller's ranks (e.g. a ctypes wrapper of ncclAllReduce on its RCCL communicator); None = torch.distributed (default)
        self._allreduce_cb = None
        if allreduce_fn is not None:
            self.set_allreduce(allreduce_fn)
        # ARD kernel (one lengthscale per input dimension, gdrf_set_ard): "log_lengthscale" is then the (D,) segment of the parameter
        # vector that exists only in ARD contexts; slot 0 stays 0 and receives a zero gradient
        self.ard = bool(ard)
        if self.ard:
            _lib.check(self.lib.gdrf_set_ard(self.ctx, 1), "gdrf_set_ard")
        # Periodic kernel (gdrf_set_period_count): "log_period" is a segment of 1 or D log-periods
        self.period_count = int(period_count) if kernel == "periodic" else 0
        if kernel == "periodic":
            if self.period_count not in (1, self.D):
                raise ValueError(f"period_count must be 1 or D = {self.D}")
            _lib.check(self.lib.gdrf_set_period_count(self.ctx, self.period_count), "gdrf_set_period_count")
        # Product kernel (gdrf_set_product): ``product`` lists the leaf factors as dicts {"name": pyro path ("kern0", "kern0.kern1"; "" for
        # a lone kernel on a subset of the axes), "kind": "rbf" | "periodic", "active_dims", "lengthscales": 1 or len(active_dims),
        # "periods": 0 for RBF, 1 or len(active_dims)}.  Each factor's parameters are views "<name>.log_variance", "<name>.log_lengthscale",
        # "<name>.log_period" ("log_variance", ... for the name "") into the three segments of gdrf_product_layout.
        self.product = self._set_product(product) if kernel == "product" else None
        # trainable mean_function parameters (gdrf_set_mean_params): {name: shape} in order, one segment of the parameter vector; their
        # sums of d elbo / d theta are written by the host into the last doubles of red_d (_write_mean_grads)
        self.mean_shapes = {str(k): torch.Size(v) for k, v in (mean_params or {}).items()}
        self.mean_count = sum(math.prod(v) for v in self.mean_shapes.values())
        if self.mean_count:
            _lib.check(self.lib.gdrf_set_mean_params(self.ctx, self.mean_count), "gdrf_set_mean_params")
        # fixed_inducing_points=False of the reference: Z = sigmoid(unconstrained block), refreshed before every evaluation
        self.learn_inducing = bool(learn_inducing)
        if self.learn_inducing:
            _lib.check(self.lib.gdrf_set_learn_inducing(self.ctx, 1), "gdrf_set_learn_inducing")
        self.whiten = bool(whiten)
        if not self.whiten:
            _lib.check(self.lib.gdrf_set_whiten(self.ctx, 0), "gdrf_set_whiten")
        # the library's offsets, asked once after every gdrf_set_* above, and the one table of the learnt parameters built from them
        raw = {}
        for key, size in (("param", 7), ("inducing", 2), ("ard", 2), ("periodic", 2), ("product", 6), ("mean", 2)):
            out = (C.c_int64 * size)()
            fn = "gdrf_mean_param_layout" if key == "mean" else f"gdrf_{key}_layout"
            _lib.check(getattr(self.lib, fn)(self.ctx, out), fn)
            raw[key] = tuple(out)
        lay = raw["param"]
        self.table = param_table(self.K, self.M, self.V, self.D, kernel, ard=self.ard, period_count=self.period_count, product=self.product,
                                 learn_inducing=self.learn_inducing, mean_shapes=self.mean_shapes, raw=raw)
        # name -> offset: the fixed slots of every context, then whatever the table places elsewhere or adds
        self.layout = dict(log_lengthscale=lay[0], log_variance=lay[1], log_noise=lay[2], log_scale_mixture=3, u_loc=lay[3], phi_unc=lay[4],
                           u_scale_tril_unc=lay[5], inducing_unc=raw["inducing"][0], total=lay[6])
        if self.mean_count:
            self.layout["mean"] = raw["mean"][0]
        self.layout.update({n: o for n, (o, _) in self.table.items()})
        red = (C.c_int64 * 6)()
        _lib.check(self.lib.gdrf_red_layout(self.ctx, red), "gdrf_red_layout")
        self.red_layout = dict(ubar=red[0], phibar=red[1], A=red[2], GT=red[3], total_T=red[4], total_d=red[5], mean=red[5] - self.mean_count)
        z = lambda n, dt: torch.zeros(int(n), dtype=dt, device=self.device)
        self.params = z(lay[6], dtype)
        self.grads = z(lay[6], dtype)
        self.exp_avg = z(lay[6], dtype)
        self.exp_avg_sq = z(lay[6], dtype)
        self.opt_extra = None
        self.red_T = z(red[4], dtype)
        self.red_d = z(red[5], torch.float64)
        self.out_d = z(8, torch.float64)
        self.Z: Optional[torch.Tensor] = None
        self.opt_step = 0
        self.last_jitter_level = 0
        self._ll_cache = None
        self._csr_cache = None                       # (tensor, _version, the device arrays bound for it): one CSR count matrix at a time
        self._csr_bound = False
        self._guess_level: Optional[int] = None      # jitter level of the previous step: this step starts on it speculatively
        self._probe_stream = torch.cuda.Stream(device=self.device)
        self.speculate = True
        self.prefactorize = True      # factorise for the next step right behind the optimizer update
        # a caller-supplied link (the reference's `link_function`, abstract_gdrf.py:34-50): a callable on the (K, n) tensor mu returning the
        # (K, n) topic weights; None = the softmax link fused into the row kernel.  Evaluated with torch between three library calls.
        self.link_function = None
        self._mean_vjp = None
        self._adjoints: Dict[str, torch.Tensor] = {}      # host copies of the row adjoints the mean's vector-Jacobian product reads

    def _set_product(self, product):
        table = [dict(f) for f in (product or ())]
        if not table:
            raise ValueError("Engine(kernel='product') needs a factor table (product=[...])")
        arr = (C.c_int * (8 * len(table)))()
        for f, fac in enumerate(table):
            if fac["kind"] not in PRODUCT_KINDS:
                raise ValueError(f"product factor kind must be 'rbf' or 'periodic', got {fac['kind']!r}")
            dims = [int(d) for d in fac["active_dims"]]
            row = [PRODUCT_KINDS[fac["kind"]], len(dims), int(fac["lengthscales"]), int(fac.get("periods", 0))] + dims + [0] * (4 - len(dims))
            if len(row) != 8:
                raise ValueError("a product factor reads at most 4 axes")
            for k, v in enumerate(row):
                arr[8 * f + k] = v
        _lib.check(self.lib.gdrf_set_product(self.ctx, len(table), arr), "gdrf_set_product")
        return table

    def set_allreduce(self, fn):
        """Register the step's collective behind the C ABI (gdrf_set_allreduce): ``fn(buf_ptr, count, is_double, stream_ptr)`` sums the flat
        payload in place over the caller's ranks and returns 0 / None; None unregisters (back to torch.distributed, or one rank)."""
        if fn is None:
            self._allreduce_cb = None
            _lib.check(self.lib.gdrf_set_allreduce(self.ctx, None, None), "gdrf_set_allreduce")
            return

        def _cb(buf, count, is_double, stream, user, _fn=fn):
            try:
                return int(_fn(buf, count, bool(is_double), stream) or 0)
            except Exception:
                return 1
        self._allreduce_cb = _lib.ALLREDUCE_FN(_cb)              # kept alive with the engine
        _lib.check(self.lib.gdrf_set_allreduce(self.ctx, C.cast(self._allreduce_cb, C.c_void_p), None), "gdrf_set_allreduce")

    @property
    def hyper_backward(self) -> str:
        """The form the next step uses ("tn" needs f16x3, fixed inducing inputs, an isotropic kernel other than RationalQuadratic)."""
        return "tn" if self.lib.gdrf_get_hyper_backward(self.ctx) else "f64"

    @property
    def rows_form(self) -> str:
        """The row form the steps and gdrf_predict use: "auto" (LDS forms) or "streamed"."""
        return "streamed" if self.lib.gdrf_get_rows_form(self.ctx) == 1 else "auto"

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.gdrf_ctx_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ---- parameter views (natural shapes) ---------------------------------------------------------
    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        buf = self.params if buf is None else buf
        if name not in self.table:
            if self.product is not None and name in ("log_lengthscale", "log_variance", "log_period", "log_scale_mixture"):
                names = tuple(self.table)
                raise KeyError(f"{name}: a product context's kernel parameters are {names[:names.index('log_noise')]}")
            raise KeyError(name)
        o, shape = self.table[name]
        return buf[o:o + math.prod(shape)].view(shape)

    PARAM_NAMES = ("log_lengthscale", "log_variance", "log_noise", "u_loc", "phi_unc", "u_scale_tril_unc")

    @property
    def param_names(self):
        """PARAM_NAMES (a product context: its factors' segments in place of slots 0 and 1) plus the blocks only some configurations learn
        (RationalQuadratic's scale_mixture, a Periodic kernel's period, inducing inputs, the mean_function's parameters)."""
        return tuple(self.table)

    def named_views(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        return {n: self.view(n, buf) for n in self.table}

    def set_inducing_points(self, Z: torch.Tensor):
        Z = Z.to(device=self.device, dtype=self.dtype).contiguous()
        assert Z.shape == (self.M, self.D), f"inducing points must be ({self.M},{self.D}), got {tuple(Z.shape)}"
        self.Z = Z.clone()
        if self.learn_inducing:
            # transform_to(interval(0, 1)).inv: logit of the value clamped to [tiny, 1 - eps] (torch SigmoidTransform._inverse)
            fi = torch.finfo(self.dtype)
            y = self.Z.clamp(min=fi.tiny, max=1.0 - fi.eps)
            self.view("inducing_unc").copy_(y.log() - (-y).log1p())

    def refresh_inducing(self):
        """Z = sigmoid(unconstrained block) when the inducing inputs are learnable (no-op otherwise)."""
        if self.learn_inducing:
            torch.sigmoid(self.view("inducing_unc"), out=self.Z)

    def set_dirichlet(self, alpha: torch.Tensor):
        a = alpha.detach().to("cpu", torch.float64).contiguous()
        assert a.shape == (self.K, self.V)
        arr = (C.c_double * (self.K * self.V))(*a.flatten().tolist())
        _lib.check(self.lib.gdrf_set_dirichlet(self.ctx, arr), "gdrf_set_dirichlet")

    # ---- workspace access for parity tests ----------------------------------------------------------
    def workspace(self, name: str, n_rows: Optional[int] = None) -> torch.Tensor:
        """Copy of a workspace buffer in its natural (unpadded) shape."""
        ptr, cnt = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.gdrf_ws_ptr(self.ctx, _WS_IDS[name], C.byref(ptr), C.byref(cnt)), "gdrf_ws_ptr")
        esz = self.lib.gdrf_ws_elem_size(self.ctx, _WS_IDS[name])
        flat = torch.empty(cnt.value, dtype=torch.float32 if esz == 4 else torch.float64, device=self.device)
        _lib.check(self.lib.gdrf_ws_copy(self.ctx, _WS_IDS[name], flat.data_ptr(), cnt.value, _stream_ptr(self.device)),
                   "gdrf_ws_copy")
        torch.cuda.synchronize(self.device)
        Mp = (self.M + 31) // 32 * 32
        ldk = (self.n_cap + 3) // 4 * 4
        n = self.n_cap if n_rows is None else n_rows
        if name in ("W", "Wbar", "Knm"):
            return flat.view(self.n_cap, Mp)[:n, :self.M].clone()
        if name in ("q", "asum"):
            return flat[:n].clone()
        if name in ("loc", "tt", "vbar", "locbar", "mu", "g_locbar"):
            return flat.view(self.K, ldk)[:, :n].clone()
        if name in ("Kuu", "L", "Linv", "LinvT"):
            return flat.view(Mp, Mp)[:self.M, :self.M].clone()
        if name in ("S", "B", "ST"):
            return flat.view(self.K, Mp, Mp)[:, :self.M, :self.M].clone()
        if name == "phi":
            return flat.view(self.K, self.V).clone()
        raise KeyError(name)

    TIMING_SLOTS = ("probe", "k_nm", "transforms", "fwd_w", "loc", "fwd_t", "elbo_rows", "bwd_wbar", "bwd_knm",
                    "tn_sym", "tn_gt", "slab_reduce", "ubar", "step_finish", "adam", "factorize")

    def set_timing(self, enable: bool):
        _lib.check(self.lib.gdrf_set_timing(self.ctx, 1 if enable else 0), "gdrf_set_timing")

    def get_timing(self) -> Dict[str, Dict[str, float]]:
        n = len(self.TIMING_SLOTS)
        ms, cnt = (C.c_double * n)(), (C.c_int64 * n)()
        _lib.check(self.lib.gdrf_get_timing(self.ctx, ms, cnt, n), "gdrf_get_timing")
        return {name: dict(ms=ms[i], count=cnt[i]) for i, name in enumerate(self.TIMING_SLOTS)}

    # gdrf_last_forms slots (include/gdrf_hip.h) and the names of their codes; the slots without names are counts
    FORM_SLOTS = ("wbar", "wbar_nslice", "a_k", "a_k_kgroups", "fwd_t", "fwd_t_kg", "loc", "ubar_q4", "rows", "rows_kt", "rows_vt", "gt",
                  "hyper", "predict", "predict_nb", "mm_chain", "mm_sbar")
    FORM_NAMES = dict(wbar=("gemm_nt", "gemm_nt_t", "split<1>", "split<2>", "split_cc", "k64", "w1"), a_k=("gemm_tn", "tn_split", "tn_topics", "w2"),
                      fwd_t=("gemm_nt", "q4", "cc", "w1"), loc=("rows", "gemm_nt", "gemm_nt_wide"), rows=("mfma", "thread", "streamed"),
                      gt=("gemm_tn", "tn_split"), hyper=("f64", "tn"), predict=("mfma", "rows_lds", "rows_mem", "rows_bigk", "streamed"),
                      mm_chain=("direct", "split8"), mm_sbar=("direct", "split8"))

    def last_forms(self) -> Dict[str, object]:
        """The kernel form each stage that the library picks from K, Mp or n launched in the most recent call that ran it
        (gdrf_last_forms): names for the form slots, counts for the others; stages that have not run yet are left out."""
        n = len(self.FORM_SLOTS)
        arr = (C.c_int * n)()
        _lib.check(self.lib.gdrf_last_forms(self.ctx, arr, n), "gdrf_last_forms")
        out = {}
        for slot, v in zip(self.FORM_SLOTS, arr):
            if v:
                out[slot] = self.FORM_NAMES[slot][v - 1] if slot in self.FORM_NAMES else v
        return out

    def last_quant_plan(self) -> Dict[str, int]:
        """(rows per workgroup pass, components per pass, dynamic LDS bytes) of the most recent predict_quant launch
        (gdrf_quant_last_plan), as a dict with the keys RP, CP and lds; zeros before the first call."""
        arr = (C.c_int * 3)()
        _lib.check(self.lib.gdrf_quant_last_plan(self.ctx, arr), "gdrf_quant_last_plan")
        return dict(RP=arr[0], CP=arr[1], lds=arr[2])

    def last_loo_plan(self) -> Dict[str, int]:
        """(rows per workgroup pass, dynamic LDS bytes) of the most recent predict_loo or psis_rows launch (gdrf_loo_last_plan,
        csrc/forms.h::loo_plan), as a dict with the keys RP and lds; zeros before the first call."""
        arr = (C.c_int * 2)()
        _lib.check(self.lib.gdrf_loo_last_plan(self.ctx, arr), "gdrf_loo_last_plan")
        return dict(RP=arr[0], lds=arr[1])

    # ---- primitives ------------------------------------------------------------------------------
    def _chk_rows(self, xs: torch.Tensor, ws: Optional[torch.Tensor] = None):
        if xs.device != self.device or xs.dtype != self.dtype or not xs.is_contiguous() or xs.dim() != 2 or xs.shape[1] != self.D:
            raise ValueError(f"xs must be a contiguous ({'n'},{self.D}) {self.dtype} tensor on {self.device}")
        if ws is not None and is_sparse_counts(ws):
            check_counts(ws, xs.shape[0], self.V, self.device)
        elif ws is not None:
            if ws.device != self.device or ws.dtype != torch.int32 or not ws.is_contiguous() or ws.shape != (xs.shape[0], self.V):
                raise ValueError(f"ws must be a contiguous (n,{self.V}) int32 tensor on {self.device}")

    def _counts_ptr(self, ws: Optional[torch.Tensor]):
        """What the library takes as ``ws_dev``: the address of a dense count matrix (any binding cleared), or None with the CSR tensor
        ``ws`` bound (gdrf_bind_counts_csr).  The int64 / int32 index arrays and the column grouping - CSR positions in (column, row) order
        by a stable sort of the column indices, and their column pointers - are built once per tensor object and ``_version``, as
        ``_ll_cache`` does for the data constant."""
        if ws is None or not is_sparse_counts(ws):
            if self._csr_bound:
                _lib.check(self.lib.gdrf_bind_counts_csr(self.ctx, None, None, None, 0, 0, None, None), "gdrf_bind_counts_csr")
                self._csr_bound = False
            return None if ws is None else ws.data_ptr()
        c = self._csr_cache
        if c is None or c[0] is not ws or c[1] != ws._version:
            crow = ws.crow_indices().to(torch.int64).contiguous()
            col = ws.col_indices().to(torch.int32).contiguous()
            val = ws.values().contiguous()
            order = torch.sort(col, stable=True)
            cperm = order.indices.to(torch.int64).contiguous()
            # ccol[v] = the number of entries with a column < v (no host read: a mini-batch step stays asynchronous)
            ccol = torch.searchsorted(order.values, torch.arange(self.V + 1, dtype=torch.int32, device=self.device)).to(torch.int64).contiguous()
            c = self._csr_cache = (ws, ws._version, (crow, col, val, ccol, cperm))
            self._csr_bound = False
        if not self._csr_bound:
            crow, col, val, ccol, cperm = c[2]
            _lib.check(self.lib.gdrf_bind_counts_csr(self.ctx, crow.data_ptr(), col.data_ptr(), val.data_ptr(), ws.shape[0], col.numel(),
                                                     ccol.data_ptr(), cperm.data_ptr()), "gdrf_bind_counts_csr")
            self._csr_bound = True
        return None

    def knm(self, xs: torch.Tensor) -> torch.Tensor:
        """K_nm = k(xs, Z) (n, M) row-major: the HBM-roofline kernel."""
        self._chk_rows(xs)
        out = torch.empty(xs.shape[0], self.M, dtype=self.dtype, device=self.device)
        self.knm_into(xs, out)
        return out

    def knm_into(self, xs: torch.Tensor, out: torch.Tensor):
        _lib.check(self.lib.gdrf_knm(self.ctx, xs.data_ptr(), xs.shape[0], self.Z.data_ptr(), self.params.data_ptr(),
                                     out.data_ptr(), out.shape[1], _stream_ptr(self.device)), "gdrf_knm")

    def fill_eps(self, seed: int, step: int, n_offset: int, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is None:
            out = torch.empty(self.K, n, dtype=self.dtype, device=self.device)
        _lib.check(self.lib.gdrf_fill_eps(self.ctx, seed & (2 ** 64 - 1), step & 0xFFFFFFFF, n_offset, n, out.data_ptr(),
                                          _stream_ptr(self.device)), "gdrf_fill_eps")
        return out

    def ll_const_dev(self, ws: torch.Tensor) -> torch.Tensor:
        """Device scalar holding the data-only constant of Multinomial.log_prob for ``ws`` (no host sync).  Cached for the
        IDENTICAL tensor object only (held here, so its storage cannot be handed to another mini-batch) at the same
        ``_version``: a fresh same-shaped mini-batch (train_script.py:461-465) is always recomputed."""
        c = self._ll_cache
        if c is not None and c[0] is ws and c[1] == ws._version:
            return c[2]
        out = torch.empty(1, dtype=torch.float64, device=self.device)
        if is_sparse_counts(ws):
            check_counts(ws, None, self.V, self.device)
        _lib.check(self.lib.gdrf_ll_const_dev(self.ctx, self._counts_ptr(ws), ws.shape[0], out.data_ptr(), _stream_ptr(self.device)),
                   "gdrf_ll_const_dev")
        self._ll_cache = (ws, ws._version, out)
        return out

    def ll_const(self, ws: torch.Tensor) -> float:
        return float(self.ll_const_dev(ws).item())

    def jitter_total(self, level: int) -> float:
        return sum(self.jitter * (10 ** n) for n in range(level + 1))

    def factorize(self, force_level: Optional[int] = None) -> int:
        """jittercholesky: smallest level whose cumulative jitter lets the Cholesky factorisation succeed IN THE
        ARRAY PRECISION (every call starts from level 0, as the reference rebuilds K_uu each time; up to 8 levels
        are attempted concurrently per launch), then the factor and its inverse in the solve precision."""
        s = _stream_ptr(self.device)
        failed = C.c_int()
        level = self._probe_level(s) if force_level is None else force_level
        while level < self.maxjitter:
            _lib.check(self.lib.gdrf_factorize(self.ctx, self.Z.data_ptr(), self.params.data_ptr(), self.jitter_total(level), s),
                       "gdrf_factorize")
            _lib.check(self.lib.gdrf_chol_failed(self.ctx, C.byref(failed), s), "gdrf_chol_failed")
            if not failed.value:
                self.last_jitter_level = level
                return level
            if force_level is not None:
                break
            level = self._probe_level(s, level + 1)      # the f64 factorisation failed where the f32 probe passed: the next level
        raise RuntimeError("reached max jitter, covariance is unstable")

    def loss_and_grads(self, xs, ws, eps, n_global: Optional[int] = None, ll_const: Optional[float] = None,
                       force_level: Optional[int] = None, renyi_alpha: Optional[float] = None, mean: Optional[torch.Tensor] = None,
                       xs_guide: Optional[torch.Tensor] = None, mean_guide: Optional[torch.Tensor] = None, mean_vjp=None):
        """One ELBO evaluation + backward.  Leaves d loss/d unconstrained in self.grads (device) and
        returns nothing host-side; call read_out() for the loss.  ``mean``: the values of the model's mean_function on these
        rows, broadcastable to (K, n) (gdrf/models/sparse_gdrf.py:346,395); None = zero_mean.  ``xs_guide``: the inputs the
        GUIDE's predictive is evaluated at when they differ from the model's (quirk Q3: the reference's guide scales twice,
        sparse_gdrf.py:376-380), with ``mean_guide`` the mean_function values there; None = the same inputs (one evaluation).
        ``mean_vjp(adj, adj_guide)`` (engines with mean_params): called after every particle's local evaluation with the (K, n) row
        adjoints d elbo / d mean of the model-side values and, with ``xs_guide``, of the guide-side ones (else None); returns the flat
        (mean_count,) vector-Jacobian product for the mean parameters' segment.  None: that segment's gradient is 0."""
        self._chk_rows(xs, ws)
        self._mean_vjp = mean_vjp if self.mean_count else None
        n = xs.shape[0]
        self._set_mean(mean, n)
        self._xs_guide = None
        if xs_guide is not None:
            self._chk_rows(xs_guide)
            if xs_guide.shape != xs.shape:
                raise ValueError("xs_guide must have the shape of xs")
            self._xs_guide = xs_guide
            self._set_mean(mean_guide, n, guide=True)
        if eps.dim() == 2:
            eps = eps.unsqueeze(0)
        P = eps.shape[0]                          # particles (Trace_ELBO num_particles): the estimator is their mean
        if tuple(eps.shape[1:]) != (self.K, n) or eps.dtype != self.dtype or not eps.is_contiguous() or eps.device != self.device:
            raise ValueError(f"eps must be a contiguous ([P,]{self.K},{n}) {self.dtype} tensor on {self.device}")
        s = _stream_ptr(self.device)
        self.refresh_inducing()
        if ll_const is None:
            llc = self.ll_const_dev(ws)
        else:
            llc = torch.full((1,), float(ll_const), dtype=torch.float64, device=self.device)
        ng = float(n if n_global is None else n_global)
        self._speculated(lambda: self._local_and_finish(xs, ws, eps, P, n, ng, llc, s, renyi_alpha), force_level)
        self._guess_level = self.last_jitter_level if force_level is None else None
        self._mean_vjp = None

    def _set_mean(self, mean, n: int, guide: bool = False):
        fn = self.lib.gdrf_set_mean_guide if guide else self.lib.gdrf_set_mean
        if mean is None:
            setattr(self, "_mean_g" if guide else "_mean", None)
            _lib.check(fn(self.ctx, None, 0, 0), "gdrf_set_mean")
            return
        mean = torch.as_tensor(mean).detach().to(device=self.device, dtype=self.dtype)
        try:
            mean = mean.expand(self.K, n)                       # (n,), (K, 1), (K, n), scalars: torch broadcasting, as f_loc + mean
        except RuntimeError:
            raise ValueError(f"mean_function returned shape {tuple(mean.shape)}, not broadcastable to ({self.K}, {n})") from None
        setattr(self, "_mean_g" if guide else "_mean", mean)    # keeps the storage alive while the context borrows it
        _lib.check(fn(self.ctx, mean.data_ptr(), mean.stride(0), mean.stride(1)), "gdrf_set_mean")

    @contextlib.contextmanager
    def _borrowed_mean(self, mean, n: int):
        """The context borrows ``mean`` inside the block and keeps none behind (a step sets its own)."""
        self._set_mean(mean, n)
        try:
            yield
        finally:
            self._set_mean(None, n)

    def _probe_level(self, stream_ptr: int, start: int = 0) -> int:
        """First cumulative-jitter level >= start whose array-precision Cholesky succeeds (probe only; raises past maxjitter)."""
        level = start
        while level < self.maxjitter:
            nlev = min(4 if level == 0 else 8, self.maxjitter - level)
            jit = (C.c_double * nlev)(*[self.jitter_total(level + l) for l in range(nlev)])
            flags = (C.c_int * nlev)()
            _lib.check(self.lib.gdrf_probe(self.ctx, self.Z.data_ptr(), self.params.data_ptr(), jit, nlev, flags, stream_ptr), "gdrf_probe")
            ok = [l for l in range(nlev) if not flags[l]]
            if ok:
                return level + ok[0]
            level += nlev
        raise RuntimeError("reached max jitter, covariance is unstable")

    def _local_and_finish(self, xs, ws, eps, P, n, ng, llc, s, renyi_alpha=None):
        """The N-side kernels for every particle, the particle combination, the all-reduce and the replicated epilogue.
        Trace_ELBO averages the P payloads (every entry is linear in the per-particle sums).  RenyiELBO(alpha) weights them
        with w_p = softmax_p((1 - alpha) e_p), e_p = the particle-varying part of the scaled ELBO (site + likelihood sums
        over ALL ranks; the terms shared by the particles factor out of the logsumexp), and reports
        -(logsumexp((1 - alpha) e_p) - log P) / (1 - alpha) through the payload's site slot.  All on the device."""
        dist_on = self._distributed()
        if dist_on:
            import torch.distributed as dist
            pg = None if isinstance(self.pg, str) else self.pg
        if renyi_alpha is not None and float(renyi_alpha) == 1.0:
            raise ValueError("RenyiELBO: alpha must differ from 1")
        Ts, ds = [], []
        xg = getattr(self, "_xs_guide", None)
        for p in range(P):
            if self.link_function is not None:
                if xg is not None:
                    raise NotImplementedError("a custom link_function together with a non-unit world's doubly scaled guide (quirk Q3)")
                self._step_local_link(xs, ws, eps[p], n, s)
            elif xg is None:
                _lib.check(self.lib.gdrf_step_local(self.ctx, xs.data_ptr(), self._counts_ptr(ws), eps[p].data_ptr(), n, self.Z.data_ptr(),
                                                    self.params.data_ptr(), self.red_T.data_ptr(), self.red_d.data_ptr(), s),
                           "gdrf_step_local")
            else:
                _lib.check(self.lib.gdrf_step_local2(self.ctx, xs.data_ptr(), xg.data_ptr(), self._counts_ptr(ws), eps[p].data_ptr(), n,
                                                     self.Z.data_ptr(), self.params.data_ptr(), self.red_T.data_ptr(),
                                                     self.red_d.data_ptr(), s), "gdrf_step_local2")
            if self.mean_count:
                self._write_mean_grads(n, xg is not None)
            if renyi_alpha is not None:
                Ts.append(self.red_T.clone()); ds.append(self.red_d.clone())
            elif P > 1:                                           # Trace_ELBO: a running sum of the payloads, no per-particle copies
                if p == 0:
                    accT, accd = self.red_T.clone(), self.red_d.clone()
                else:
                    accT.add_(self.red_T); accd.add_(self.red_d)
        if renyi_alpha is not None:
            T_all, d_all = torch.stack(Ts), torch.stack(ds)
            e = d_all[:, 0] + d_all[:, 1]                         # this rank's site + likelihood sums per particle
            if dist_on:
                dist.all_reduce(e, group=pg)
            logw = (1.0 - float(renyi_alpha)) * e / ng
            w = torch.softmax(logw, 0)
            self.red_T.copy_((w.to(T_all.dtype)[:, None] * T_all).sum(0))
            self.red_d.copy_((w[:, None] * d_all).sum(0))
            bound = (torch.logsumexp(logw, 0) - math.log(P)) / (1.0 - float(renyi_alpha))      # scaled by 1/N already
            # step_finish forms loss = -(red_d[0] + red_d[1] + constants) / N from the REDUCED payload: one rank carries it
            first = (not dist_on) or dist.get_rank(pg) == 0
            self.red_d[0] = bound * ng if first else 0.0
            self.red_d[1] = 0.0
        elif P > 1:
            self.red_T.copy_(accT.div_(P))
            self.red_d.copy_(accd.div_(P))
        self.red_d[7:8].copy_(llc)                   # the data constant is a sum over observations too; stays on the device
        if self._allreduce_cb is not None:           # the caller's collective, behind the C ABI (pack, its sum over the ranks, unpack)
            _lib.check(self.lib.gdrf_payload_allreduce(self.ctx, self.red_T.data_ptr(), self.red_d.data_ptr(), s), "gdrf_payload_allreduce")
        elif dist_on:
            # ONE collective per step: the doubles of red_d ride in the tail of the flat payload (exactly in float64 contexts; as four
            # float pieces each in float32 ones: exact over <= 8 ranks for the loss sums, whose per-rank values have similar magnitude,
            # and to 2^-24 of the largest summand for entries that differ by orders of magnitude between ranks - csrc/kernels_n.h)
            _lib.check(self.lib.gdrf_payload_pack(self.ctx, self.red_T.data_ptr(), self.red_d.data_ptr(), s), "gdrf_payload_pack")
            dist.all_reduce(self.red_T, group=pg)    # RCCL over xGMI (backend "nccl" on ROCm)
            _lib.check(self.lib.gdrf_payload_unpack(self.ctx, self.red_T.data_ptr(), self.red_d.data_ptr(), s), "gdrf_payload_unpack")
        self._finish(ng, None)

    def _adjoint(self, which: str, n: int) -> torch.Tensor:
        """(K, n) view of a copy of a row-adjoint workspace, enqueued on the current stream (no host synchronisation)."""
        buf = self._adjoints.get(which)
        ldk = (self.n_cap + 3) // 4 * 4
        if buf is None:
            buf = self._adjoints[which] = torch.empty(self.K, ldk, dtype=self.dtype, device=self.device)
        _lib.check(self.lib.gdrf_ws_copy(self.ctx, _WS_IDS[which], buf.data_ptr(), buf.numel(), _stream_ptr(self.device)), "gdrf_ws_copy")
        return buf[:, :n]

    def _write_mean_grads(self, n: int, two_point: bool):
        """This particle's sums of d elbo / d theta of the mean parameters -> the mean segment of red_d, before the particle combination
        and the collective.  The mean enters mu where f_loc does, so its row adjoint is the row kernel's locbar (guide side: g_locbar)."""
        seg = self.red_d[self.red_layout["mean"]:]
        if self._mean_vjp is None:
            seg.zero_()
            return
        g = self._mean_vjp(self._adjoint("locbar", n), self._adjoint("g_locbar", n) if two_point else None)
        seg.copy_(g.reshape(-1))

    def _step_local_link(self, xs, ws, eps_p, n: int, s: int):
        """gdrf_step_local with the link and its Jacobian evaluated here: theta = link(mu) and mubar = J^T thetabar by autograd
        (sparse_gdrf.py:361: `topic_probs = self._link_function(mu).transpose(-2, -1)`)."""
        args = (self.ctx, xs.data_ptr(), self._counts_ptr(ws), eps_p.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(),
                self.red_T.data_ptr(), self.red_d.data_ptr(), s)
        _lib.check(self.lib.gdrf_step_local_link(*args, 0, None, 0), "gdrf_step_local_link(0)")
        mu = self.workspace("mu", n).requires_grad_(True)                      # (K, n)
        with torch.enable_grad():
            theta = self.link_function(mu)
        if tuple(theta.shape) != (self.K, n):
            raise ValueError(f"link_function returned shape {tuple(theta.shape)}, expected ({self.K}, {n}) like its argument")
        th = theta.detach().to(self.dtype).contiguous()
        _lib.check(self.lib.gdrf_step_local_link(*args, 1, th.data_ptr(), n), "gdrf_step_local_link(1)")
        thbar = self.workspace("locbar", n)
        if theta.requires_grad:
            (mubar,) = torch.autograd.grad(theta, mu, grad_outputs=thbar.to(theta.dtype))
        else:                                                                  # a link that ignores mu
            mubar = torch.zeros_like(mu)
        mubar = mubar.detach().to(self.dtype).contiguous()
        _lib.check(self.lib.gdrf_step_local_link(*args, 2, mubar.data_ptr(), n), "gdrf_step_local_link(2)")

    def _distributed(self) -> bool:
        if self.pg is None:
            return False
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return False
        pg = None if isinstance(self.pg, str) else self.pg
        return dist.get_world_size(pg) > 1

    def _finish(self, n_global: float, ll_const: Optional[float]):
        s = _stream_ptr(self.device)
        if ll_const is None:                         # the reduced copy travels in red_d[7]; the kernel reads it there (no host sync)
            ll_const = float("nan")
        _lib.check(self.lib.gdrf_step_finish(self.ctx, self.Z.data_ptr(), self.params.data_ptr(), self.red_T.data_ptr(),
                                             self.red_d.data_ptr(), n_global, ll_const, self.grads.data_ptr(),
                                             self.out_d.data_ptr(), s), "gdrf_step_finish")

    def adam(self, mode: str, lr: float, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=10.0):
        self.opt_step += 1
        _lib.check(self.lib.gdrf_adam(self.ctx, OPT_MODES[mode], self.params.data_ptr(), self.grads.data_ptr(),
                                      self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.opt_step, lr, betas[0], betas[1],
                                      eps, weight_decay, clip, _stream_ptr(self.device)), "gdrf_adam")
        self._prefactorize()

    def segments(self) -> Dict[str, tuple]:
        """{name: (offset, length)} of every learnt parameter tensor in the flat vector (the segments of optim_step)."""
        return {n: (o, math.prod(shape)) for n, (o, shape) in self.table.items()}

    def state_buffer(self, slot: int) -> torch.Tensor:
        """Optimizer state vector 1 (exp_avg), 2 (exp_avg_sq) or 3 (opt_extra, allocated on first use)."""
        if slot == 3 and self.opt_extra is None:
            self.opt_extra = torch.zeros_like(self.params)
        return (self.exp_avg, self.exp_avg_sq, self.opt_extra)[slot - 1]

    def optim_step(self, rule: str, segs):
        """One update of ``segs`` (gdrf_optim_step): a sequence of dicts {offset, length, a (up to 8 scalars of this step, include/gdrf_hip.h),
        flags, clip_norm, clip_value}, one per parameter tensor.  The state vectors are exp_avg, exp_avg_sq and opt_extra; elements outside
        every segment do not change.  Counts the step and queues the next factorisation like adam()."""
        arr = (_lib.OptSeg * max(1, len(segs)))()
        for k, sg in enumerate(segs):
            e = arr[k]
            e.offset, e.length = int(sg["offset"]), int(sg["length"])
            e.flags = int(sg.get("flags", 0))
            e.clip_norm, e.clip_value = float(sg.get("clip_norm", 0.0)), float(sg.get("clip_value", 0.0))
            for j, x in enumerate(sg["a"]):
                e.a[j] = float(x)
        s3 = self.opt_extra.data_ptr() if self.opt_extra is not None else None
        self.opt_step += 1
        _lib.check(self.lib.gdrf_optim_step(self.ctx, OPT_RULES[rule], C.cast(arr, C.c_void_p), len(segs), self.params.data_ptr(),
                                            self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), s3,
                                            _stream_ptr(self.device)), "gdrf_optim_step")
        self._prefactorize()

    def _prefactorize(self):
        """The next step's factorisation, queued right behind the optimizer update."""
        # The next step's factorisation depends only on what this update just wrote (kernel hyper-parameters, inducing inputs): start it now,
        # on the guessed jitter level, so that its serial chain runs while the host reads the loss and enqueues the step.  The step checks
        # on the device that the inputs are still the same (anything may write the parameters in between) and redoes itself otherwise.
        if self.speculate and self.prefactorize and self._guess_level is not None:
            self.refresh_inducing()
            _lib.check(self.lib.gdrf_factorize_mode(self.ctx, self.Z.data_ptr(), self.params.data_ptr(), self.jitter_total(self._guess_level),
                                                    _stream_ptr(self.device), 1), "gdrf_factorize_mode")

    def read_out(self) -> Dict[str, float]:
        o = self.out_d.cpu().tolist()          # synchronises
        return dict(loss=o[0], chol_failed=o[1], site=o[2], loglik=o[3], lp_phi=o[4])

    def predict(self, xs: torch.Tensor, mode: int, ws: Optional[torch.Tensor] = None):
        """Predictive path (gdrf_predict): mode 0 f_loc (K, n), 1 topic_probs (n, K), 2 word_probs (n, V), 3 {sum w log p, sum w},
        4 (f_loc, f_var) as (2, K, n).  Like the step, it starts on the previous jitter level (and on the factorisation adam() queued
        ahead, if its inputs still match) while the array-precision probe that decides the level runs on the second stream; a wrong
        guess redoes the evaluation on the right level."""
        self._chk_rows(xs, ws)
        n = xs.shape[0]
        self.refresh_inducing()
        if mode == 4 and n > self.n_cap:
            raise ValueError(f"predict(mode=4) needs n <= n_cap ({n} > {self.n_cap})")

        def run():
            out = None
            if mode == 0:
                out = torch.empty(self.K, n, dtype=self.dtype, device=self.device)
            elif mode == 1:
                out = torch.empty(n, self.K, dtype=self.dtype, device=self.device)
            elif mode == 2:
                out = torch.empty(n, self.V, dtype=self.dtype, device=self.device)
            elif mode == 4:          # (f_loc, f_var) of gp.util.conditional(full_cov=False): sparse_gdrf.py:277-319
                out = torch.empty(2, self.K, n, dtype=self.dtype, device=self.device)
            _lib.check(self.lib.gdrf_predict(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(),
                                             self._counts_ptr(ws) if mode == 3 else None, mode,
                                             out.data_ptr() if out is not None else None, self.out_d.data_ptr(),
                                             _stream_ptr(self.device)), "gdrf_predict")
            return self.out_d[:2].clone() if mode == 3 else out

        return self._speculated(run)

    def _speculated(self, run, force_level: Optional[int] = None):
        """``run()`` under the jitter-level protocol of the step and the predictive calls.  Speculate on the previous step's level: the
        solve-precision factorisation and ``run()`` go onto the main stream at once, the array-precision probe (which decides the level, as
        the reference's fp32 jittercholesky would) runs beside them on a second stream, and the host only waits for the probe and for the
        factorisation flag while the GPU is busy with ``run()``'s kernels.  A wrong guess (the level moved, or the f64 factorisation failed
        where the f32 one passed) redoes ``run()`` on the right level; every rank holds the same parameters, so every rank takes the same
        branch.  ``force_level`` (or no previous level, or ``speculate`` off): factorise on that level first, then ``run()``."""
        guess = self._guess_level if (force_level is None and self.speculate) else None
        if guess is None:
            self.factorize(force_level)
            return run()
        main = torch.cuda.current_stream(self.device)
        self._probe_stream.wait_stream(main)
        ps = self._probe_stream.cuda_stream
        # the probe of the first levels goes out FIRST, without waiting: it runs while the host enqueues run()
        nlev0 = min(4, self.maxjitter)
        jit0 = (C.c_double * nlev0)(*[self.jitter_total(l) for l in range(nlev0)])
        _lib.check(self.lib.gdrf_probe_launch(self.ctx, self.Z.data_ptr(), self.params.data_ptr(), jit0, nlev0, ps), "gdrf_probe_launch")
        # mode 2: a factorisation made ahead of this call (behind the previous optimizer update, see adam()) is reused after a
        # device-side check that its inputs are still the current ones; gdrf_chol_failed reports a mismatch like a failure
        _lib.check(self.lib.gdrf_factorize_mode(self.ctx, self.Z.data_ptr(), self.params.data_ptr(), self.jitter_total(guess),
                                                main.cuda_stream, 2), "gdrf_factorize_mode")
        fact_done = torch.cuda.Event()
        fact_done.record(main)
        out = run()
        flags0 = (C.c_int * nlev0)()
        _lib.check(self.lib.gdrf_probe_read(self.ctx, nlev0, flags0, ps), "gdrf_probe_read")
        ok0 = [l for l in range(nlev0) if not flags0[l]]
        level = ok0[0] if ok0 else self._probe_level(ps, start=nlev0)
        failed = C.c_int()
        self._probe_stream.wait_event(fact_done)
        _lib.check(self.lib.gdrf_chol_failed(self.ctx, C.byref(failed), ps), "gdrf_chol_failed")
        if level == guess and not failed.value:
            self.last_jitter_level = level
            return out
        torch.cuda.synchronize(self.device)
        self.factorize(None)
        self._guess_level = self.last_jitter_level
        return run()

    def _mc_seed(self, what: str, n: int, eps, seed) -> int:
        """What the Monte-Carlo predictive calls check once the rows are known: n <= n_cap, an injected ``eps`` that the kernel can read
        in place, a seed where there is none.  Returns the seed as the library takes it."""
        if n > self.n_cap:
            raise ValueError(f"{what} needs n <= n_cap ({n} > {self.n_cap})")
        if eps is not None and (eps.dtype != self.dtype or eps.device != self.device or not eps.is_contiguous()):
            raise ValueError(f"eps must be a contiguous {self.dtype} tensor on {self.device}")
        if eps is None and seed is None:
            raise ValueError(f"{what} needs a seed or an injected eps")
        return 0 if seed is None else int(seed) & (2 ** 64 - 1)

    def predict_mc(self, xs: torch.Tensor, mode: int, num_samples: int, ws: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                   row_offset: int = 0, eps: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None):
        """Monte-Carlo integration over the guide's q(mu) at the rows ``xs`` (gdrf_predict_mc, csrc/predict_mc.h): mode 0 theta samples
        (S, n, K), 1 their mean and variance (2, n, K), 2 {sum_n l_n, sum w} of the predictive score against the dense counts ``ws``, 3 mu
        samples (S, K, n).  ``eps``: an injected (S, K, n) array; None = Philox draws keyed by ``seed`` with counter (row_offset + row, topic,
        sample), so rows cut into several calls, each with its ``row_offset``, draw what one call draws.  ``mean``: the mean_function's values
        on these rows, broadcastable to (K, n).  n <= n_cap.  Same jitter-level protocol as predict()."""
        if mode not in (0, 1, 2, 3):
            raise ValueError("predict_mc: mode must be 0 (theta samples), 1 (moments), 2 (predictive score) or 3 (mu samples)")
        S = check_mc_args(num_samples, self.K, int(xs.shape[0]), eps, ws)
        if mode == 2 and ws is None:
            raise ValueError("predict_mc(mode=2) needs ws")
        self._chk_rows(xs, ws if mode == 2 else None)
        n = xs.shape[0]
        seed = self._mc_seed("predict_mc", n, eps, seed)
        self.refresh_inducing()

        def run():
            out = None
            if mode != 2:
                out = torch.empty({0: (S, n, self.K), 1: (2, n, self.K), 3: (S, self.K, n)}[mode], dtype=self.dtype, device=self.device)
            _lib.check(self.lib.gdrf_predict_mc(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(),
                                                self._counts_ptr(ws) if mode == 2 else None, mode, S, seed, int(row_offset),
                                                eps.data_ptr() if eps is not None else None, out.data_ptr() if out is not None else None,
                                                self.out_d.data_ptr(), _stream_ptr(self.device)), "gdrf_predict_mc")
            return self.out_d[:2].clone() if mode == 2 else out

        with self._borrowed_mean(mean, n):
            return self._speculated(run)

    def predict_info(self, xs: torch.Tensor, num_samples: int, seed: Optional[int] = None, row_offset: int = 0,
                     eps: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The entropy and information-gain maps at the rows ``xs`` (gdrf_predict_info, csrc/predict_info.h), (6, n) float64 in the order
        of INFO_NAMES, integrated over the ``num_samples`` draws predict_mc makes under the same ``seed`` / ``row_offset`` / ``eps`` /
        ``mean`` without storing a sample.  n <= n_cap.  Same jitter-level protocol as predict()."""
        S = check_mc_args(num_samples, self.K, int(xs.shape[0]), eps)
        self._chk_rows(xs, None)
        n = xs.shape[0]
        seed = self._mc_seed("predict_info", n, eps, seed)
        self.refresh_inducing()

        def run():
            out = torch.empty(len(INFO_NAMES), n, dtype=torch.float64, device=self.device)
            _lib.check(self.lib.gdrf_predict_info(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), S, seed,
                                                  int(row_offset), eps.data_ptr() if eps is not None else None, out.data_ptr(),
                                                  _stream_ptr(self.device)), "gdrf_predict_info")
            return out

        with self._borrowed_mean(mean, n):
            return self._speculated(run)

    def predict_score(self, xs: torch.Tensor, ws: torch.Tensor, num_samples: int, seed: Optional[int] = None, row_offset: int = 0,
                      eps: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The per-row Monte-Carlo log predictive densities of the counts ``ws`` at the rows ``xs`` (gdrf_predict_score,
        csrc/predict_score.h), (5, n) float64 in the order of SCORE_NAMES, over the ``num_samples`` draws predict_mc makes under the same
        ``seed`` / ``row_offset`` / ``eps`` / ``mean`` without storing a sample.  ``ws``: dense (n, V) int32 or ``torch.sparse_csr``; no
        V is too large.  n <= n_cap.  Same jitter-level protocol as predict()."""
        S = check_score_args(num_samples, self.K, self.V, int(xs.shape[0]), ws, eps)
        self._chk_rows(xs, ws)
        n = xs.shape[0]
        seed = self._mc_seed("predict_score", n, eps, seed)
        if is_sparse_counts(ws):
            crow, col, val = self._csr_arrays(ws)
            if col.numel() == 0:
                # An all-empty matrix: torch gives its empty index arrays no address, and the library, which cannot see on the host that
                # no entry is stored (the row pointers live on the device), insists on col_dev and val_dev.  The stand-in is never read:
                # every row has crow[n] == crow[n + 1].
                col = val = torch.zeros(1, dtype=torch.int32, device=self.device)
            counts = (None, crow.data_ptr(), col.data_ptr(), val.data_ptr())
        else:
            counts = (ws.data_ptr(), None, None, None)
        self.refresh_inducing()

        def run():
            out = torch.empty(len(SCORE_NAMES), n, dtype=torch.float64, device=self.device)
            _lib.check(self.lib.gdrf_predict_score(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), *counts, S, seed,
                                                   int(row_offset), eps.data_ptr() if eps is not None else None, out.data_ptr(),
                                                   _stream_ptr(self.device)), "gdrf_predict_score")
            return out

        with self._borrowed_mean(mean, n):
            return self._speculated(run)

    def _score_counts(self, ws: torch.Tensor):
        """(ws, crow, col, val) as gdrf_predict_score and gdrf_predict_loo take the counts, dense or CSR"""
        if not is_sparse_counts(ws):
            return (ws.data_ptr(), None, None, None), ws
        crow, col, val = self._csr_arrays(ws)
        if col.numel() == 0:      # an all-empty matrix: see predict_score
            col = val = torch.zeros(1, dtype=torch.int32, device=self.device)
        return (None, crow.data_ptr(), col.data_ptr(), val.data_ptr()), (crow, col, val)

    def predict_loo(self, xs: torch.Tensor, ws: torch.Tensor, num_samples: int, seed: Optional[int] = None, row_offset: int = 0,
                    eps: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None, return_log_lik: bool = False):
        """Pareto-smoothed importance-sampling leave-one-out of the counts ``ws`` at the rows ``xs`` (gdrf_predict_loo,
        csrc/predict_loo.h has the definition), (6, n) float64 in the order of LOO_NAMES, from the log likelihoods a_s predict_score
        forms over the same ``num_samples`` draws (``seed`` / ``row_offset`` / ``eps`` / ``mean`` as there; ``lpd``, ``total`` and
        ``log_coef`` are its, bit for bit).  LOO_MIN_SAMPLES <= num_samples <= LOO_MAX_SAMPLES.  ``return_log_lik``: also the (S, n)
        float64 matrix of the a_s, as a second result.  ``ws``: dense (n, V) int32 or ``torch.sparse_csr``; no V is too large.
        n <= n_cap.  Same jitter-level protocol as predict()."""
        S = check_loo_args(num_samples, self.K, self.V, int(xs.shape[0]), ws, eps)
        self._chk_rows(xs, ws)
        n = xs.shape[0]
        seed = self._mc_seed("predict_loo", n, eps, seed)
        counts, _keep = self._score_counts(ws)
        self.refresh_inducing()

        def run():
            out = torch.empty(len(LOO_NAMES), n, dtype=torch.float64, device=self.device)
            a = torch.empty(S, n, dtype=torch.float64, device=self.device) if return_log_lik else None
            _lib.check(self.lib.gdrf_predict_loo(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), *counts, S,
                                                 loo_tail_len(S), seed, int(row_offset), eps.data_ptr() if eps is not None else None,
                                                 out.data_ptr(), a.data_ptr() if a is not None else None, _stream_ptr(self.device)),
                       "gdrf_predict_loo")
            return (out, a) if return_log_lik else out

        with self._borrowed_mean(mean, n):
            return self._speculated(run)

    def psis_rows(self, log_lik: torch.Tensor) -> torch.Tensor:
        """The PSIS stage alone on a caller's own (S, n) float64 log-likelihood matrix on the device (gdrf_psis_rows): (3, n) float64,
        ``elpd_loo``, ``pareto_k`` and ``ess`` of every column as predict_loo forms them from its own a_s.  No model quantity is read."""
        S, n = check_psis_args(log_lik)
        if log_lik.dtype != torch.float64 or log_lik.device != self.device or not log_lik.is_contiguous():
            raise ValueError(f"log_lik must be a contiguous float64 tensor on {self.device}")
        out = torch.empty(3, n, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gdrf_psis_rows(self.ctx, log_lik.data_ptr(), S, loo_tail_len(S), n, out.data_ptr(), _stream_ptr(self.device)),
                   "gdrf_psis_rows")
        return out

    def predict_quant(self, xs: torch.Tensor, mode: int, num_samples: int, levels=None, words: Optional[torch.Tensor] = None,
                      seed: Optional[int] = None, row_offset: int = 0, eps: Optional[torch.Tensor] = None,
                      mean: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Credible-interval, exceedance and dominant-topic maps at the rows ``xs`` (gdrf_predict_quant, csrc/predict_quant.h) over the
        ``num_samples`` draws predict_mc makes under the same ``seed`` / ``row_offset`` / ``eps`` / ``mean``, float64: mode QUANT_QUANTILE
        the type-7 sample quantiles at the ``levels`` (Q, n, C), QUANT_EXCEED the share of draws strictly above each threshold of
        ``levels`` (Tn, n, C), QUANT_DOMINANT the share of draws in which each topic is the largest (n, K).  The C components are the K
        topic proportions or, with ``words`` (an int32 index tensor on the device; may repeat, any order), the chosen entries of theta Phi.
        n <= n_cap.  Same jitter-level protocol as predict()."""
        S, lv, nw = check_quant_args(mode, num_samples, self.K, self.V, int(xs.shape[0]), levels, words, eps)
        self._chk_rows(xs, None)
        n = xs.shape[0]
        if nw and (not torch.is_tensor(words) or words.device != self.device or words.dtype != torch.int32 or not words.is_contiguous()):
            raise ValueError(f"words must be a contiguous int32 tensor on {self.device}")
        seed = self._mc_seed("predict_quant", n, eps, seed)
        self.refresh_inducing()
        ncomp = nw if nw else self.K
        levels_c = (C.c_double * len(lv))(*lv) if lv else None

        def run():
            out = torch.empty((n, self.K) if mode == QUANT_DOMINANT else (len(lv), n, ncomp), dtype=torch.float64, device=self.device)
            _lib.check(self.lib.gdrf_predict_quant(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), int(mode), S, seed,
                                                   int(row_offset), eps.data_ptr() if eps is not None else None, levels_c, len(lv),
                                                   words.data_ptr() if nw else None, nw, out.data_ptr(), _stream_ptr(self.device)),
                       "gdrf_predict_quant")
            return out

        with self._borrowed_mean(mean, n):
            return self._speculated(run)

    # ---- fold-in: topic proportions of observed rows from their own counts (csrc/foldin.h) ---------------
    def _csr_arrays(self, ws: torch.Tensor):
        """(crow int64, col int32, val int32) of a CSR count matrix, contiguous, as gdrf_fold_in reads them"""
        return (ws.crow_indices().to(torch.int64).contiguous(), ws.col_indices().to(torch.int32).contiguous(), ws.values().contiguous())

    def fold_in(self, xs: torch.Tensor, ws: torch.Tensor, mode: int, num_iters: int = 64, tol: float = 1e-6,
                ws_score: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None):
        """The per-row MAP of mu given the rows' own counts ``ws`` with the GP as the prior (gdrf_fold_in, csrc/foldin.h has the
        definition): mode 0 theta_hat (n, K), 1 mu_hat (K, n), 2 the expected topic counts at theta_hat (n, K), 3 {sum w2 log p_hat, sum w2}
        for the counts ``ws_score`` (default: ``ws``).  ``ws`` / ``ws_score``: dense (n, V) int32 or ``torch.sparse_csr``, both in the same
        layout.  At most ``num_iters`` iterations per row; a row stops once |g|_inf / max(1, R) <= ``tol``.  ``mean``: the mean_function's
        values on these rows, broadcastable to (K, n).  Returns (result, diag) with diag (3, n) float64: J at the result, |g|_inf /
        max(1, R), the iterations used.  n <= n_cap.  Same jitter-level protocol as predict()."""
        if mode not in (0, 1, 2, 3):
            raise ValueError("fold_in: mode must be 0 (theta), 1 (mu), 2 (expected topic counts) or 3 (completion score)")
        num_iters, tol = check_fold_args(num_iters, tol, int(xs.shape[0]), self.V, ws, ws_score)
        if ws_score is not None and mode != 3:
            raise ValueError("fold_in: ws_score is read by mode 3 only")
        self._chk_rows(xs, ws)
        if ws_score is not None:
            self._chk_rows(xs, ws_score)
        n = xs.shape[0]
        if n > self.n_cap:
            raise ValueError(f"fold_in needs n <= n_cap ({n} > {self.n_cap})")
        sparse = is_sparse_counts(ws)
        fit = self._csr_arrays(ws) if sparse else None
        score = None if ws_score is None else (self._csr_arrays(ws_score) if sparse else ws_score)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.refresh_inducing()

        def run():
            out = None
            if mode != 3:
                out = torch.empty((self.K, n) if mode == 1 else (n, self.K), dtype=self.dtype, device=self.device)
            diag = torch.empty(3, n, dtype=torch.float64, device=self.device)
            a = (None,) + tuple(ptr(t) for t in fit) if sparse else (ws.data_ptr(), None, None, None)
            if score is None:
                b = (None, None, None, None)
            else:
                b = (None,) + tuple(ptr(t) for t in score) if sparse else (score.data_ptr(), None, None, None)
            _lib.check(self.lib.gdrf_fold_in(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), *a, *b, mode, num_iters,
                                             tol, ptr(out), diag.data_ptr(), self.out_d.data_ptr(), _stream_ptr(self.device)), "gdrf_fold_in")
            return (self.out_d[:2].clone() if mode == 3 else out), diag

        with self._borrowed_mean(mean, n):
            return self._speculated(run)

    # ---- posterior-predictive count samples (csrc/sample_counts.h) ------------------------------------
    def fill_token_uniforms(self, seed: int, num_samples: int, row_offset: int, n: int, tmax: int) -> torch.Tensor:
        """(S, n, tmax) float64: exactly the uniforms sample_counts draws inline from ``seed`` for the rows row_offset .. row_offset + n - 1
        (Philox keyed by the seed, counter (global row, 2^31 | token // 4, sample), word token % 4): the counterpart of fill_eps."""
        S, n, tmax = int(num_samples), int(n), int(tmax)
        if S < 1 or n < 1 or tmax < 0 or int(row_offset) < 0:
            raise ValueError(f"fill_token_uniforms needs num_samples >= 1, n >= 1, tmax >= 0 and row_offset >= 0, got {(num_samples, n, tmax, row_offset)}")
        out = torch.empty(S, n, tmax, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gdrf_sample_counts(self.ctx, None, n, None, None, tmax, None, 2, S, int(seed) & (2 ** 64 - 1), int(row_offset),
                                               out.data_ptr(), None, None, None, _stream_ptr(self.device)), "gdrf_sample_counts")
        return out

    def sample_counts(self, theta: torch.Tensor, totals: torch.Tensor, mode: int = 0, ws: Optional[torch.Tensor] = None,
                      seed: Optional[int] = None, row_offset: int = 0, u: Optional[torch.Tensor] = None):
        """Counts drawn from Multinomial(totals[n], theta[s, n] Phi) (gdrf_sample_counts, csrc/sample_counts.h has the definition), Phi
        from the engine's parameters.  ``theta``: (S, n, K) samples of the topic proportions in the engine's dtype; ``totals``: (n,) int32.
        mode 0: w_rep (S, n, V) int32.  mode 1: the predictive-check statistics of the same draws against the dense counts ``ws`` (n, V),
        no replicate stored: (dev (2, S) float64 = the deviances of the replicates and of ``ws`` under each draw, zeros (S, V) int64 = the
        rows in which a word was not drawn).  ``u``: injected uniforms (S, n, >= max totals) float64 in [0, 1); None = Philox draws keyed
        by ``seed`` with counter (row_offset + row, token block, sample), so rows cut into several calls, each with its ``row_offset``,
        draw what one call draws.  Any n: nothing here is held per row in the engine."""
        S, n, tmax = check_count_args(theta, totals, self.K, self.V, mode, ws, u, row_offset)
        for name, t, dt in (("theta", theta, self.dtype), ("totals", totals, torch.int32), ("ws", ws, torch.int32), ("u", u, torch.float64)):
            if t is not None and (t.dtype != dt or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} tensor on {self.device}")
        if u is None and seed is None:
            raise ValueError("sample_counts needs a seed or injected uniforms u")
        seed = 0 if seed is None else int(seed) & (2 ** 64 - 1)
        if u is not None and u.shape[2] != tmax:
            u = u[:, :, :tmax].contiguous()      # the kernel strides a row's uniforms by tmax
        if u is not None and tmax == 0:
            u = None
        out = dev = zeros = None
        if mode == 0:
            out = torch.empty(S, n, self.V, dtype=torch.int32, device=self.device)
        else:
            dev = torch.empty(2, S, dtype=torch.float64, device=self.device)
            zeros = torch.empty(S, self.V, dtype=torch.int64, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.gdrf_sample_counts(self.ctx, theta.data_ptr(), n, self.params.data_ptr(), totals.data_ptr(), tmax, ptr(ws), mode, S,
                                               seed, int(row_offset), ptr(u), ptr(out), ptr(dev), ptr(zeros), _stream_ptr(self.device)),
                   "gdrf_sample_counts")
        return out if mode == 0 else (dev, zeros)

    # ---- the joint posterior at new inputs (csrc/predict_cov.h) -----------------------------------------
    def _chk_joint_rows(self, xs: torch.Tensor, what: str) -> int:
        self._chk_rows(xs)
        n = xs.shape[0]
        if n > self.n_cap:
            raise ValueError(f"{what} needs n <= n_cap ({n} > {self.n_cap})")
        return n

    def predict_cov(self, xs: torch.Tensor, which: int = 0) -> torch.Tensor:
        """The joint posterior covariance at the rows ``xs`` (gdrf_predict_cov): which = 0 the K matrices C_k = R + (W S_k)(W S_k)^T as
        (K, n, n), 1 the topic-independent R = K_** - W W^T as (n, n); each equal to its transpose to the bit.  All rows at once:
        n <= min(n_cap, JOINT_MAX_ROWS).  Same jitter-level protocol for K_uu as predict()."""
        if which not in (0, 1):
            raise ValueError("predict_cov: which must be 0 (the K full covariances) or 1 (the residual R)")
        check_joint_args(1, self.K, self.M, int(xs.shape[0]))
        n = self._chk_joint_rows(xs, "predict_cov")
        self.refresh_inducing()

        def run():
            out = torch.empty((self.K, n, n) if which == 0 else (n, n), dtype=self.dtype, device=self.device)
            _lib.check(self.lib.gdrf_predict_cov(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), which, out.data_ptr(),
                                                 _stream_ptr(self.device)), "gdrf_predict_cov")
            return out

        return self._speculated(run)

    def sample_joint(self, xs: torch.Tensor, num_samples: int, seed: Optional[int] = None, xi: Optional[torch.Tensor] = None,
                     zeta: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(S, K, n) joint samples of the latent field at the rows ``xs`` (gdrf_sample_joint):
        f[s, k] = W (u_k + S_k xi[s, k]) + G zeta[s, k] + mean[k], G G^T = R + j I.  ``xi`` (S, K, M) / ``zeta`` (S, K, n): injected standard
        normals; None = Philox draws keyed by ``seed`` (fill_eps(seed, s, JOINT_XI_OFFSET, M) is xi[s], fill_eps(seed, s, JOINT_ZETA_OFFSET, n)
        is zeta[s]).  ``mean``: the mean_function's values on these rows, broadcastable to (K, n).  j is the cumulative jitter of the first
        level of the engine's schedule (jitter, maxjitter; cumulative as for K_uu) at which R + j I factorises without a failed pivot - a flag
        the kernel sets, read back after every attempt; ``last_joint_jitter`` / ``last_joint_level`` hold what was used.  RuntimeError when
        every level fails.  K_uu's own level follows the protocol of predict().  All rows at once: n <= min(n_cap, JOINT_MAX_ROWS)."""
        S = check_joint_args(num_samples, self.K, self.M, int(xs.shape[0]), xi, zeta)
        n = self._chk_joint_rows(xs, "sample_joint")
        for name, t in (("xi", xi), ("zeta", zeta)):
            if t is not None and (t.dtype != self.dtype or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {self.dtype} tensor on {self.device}")
        if (xi is None or zeta is None) and seed is None:
            raise ValueError("sample_joint needs a seed unless both xi and zeta are injected")
        seed = 0 if seed is None else int(seed) & (2 ** 64 - 1)
        self.refresh_inducing()
        failed = C.c_int()

        def run(jit):
            out = torch.empty(S, self.K, n, dtype=self.dtype, device=self.device)
            _lib.check(self.lib.gdrf_sample_joint(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(), S, seed,
                                                  xi.data_ptr() if xi is not None else None, zeta.data_ptr() if zeta is not None else None,
                                                  jit, out.data_ptr(), _stream_ptr(self.device)), "gdrf_sample_joint")
            return out

        with self._borrowed_mean(mean, n):
            for level in range(self.maxjitter):
                jit = self.jitter_total(level)
                if level == 0:
                    out = self._speculated(lambda: run(jit))         # settles K_uu's level as well
                else:
                    # only R + j I, its factorisation and the two sample products depend on the level: W, R, u + S xi and zeta stay in place
                    _lib.check(self.lib.gdrf_sample_joint_retry(self.ctx, n, S, jit, out.data_ptr(), _stream_ptr(self.device)),
                               "gdrf_sample_joint_retry")
                _lib.check(self.lib.gdrf_joint_failed(self.ctx, C.byref(failed), _stream_ptr(self.device)), "gdrf_joint_failed")
                if not failed.value:
                    self.last_joint_jitter, self.last_joint_level = jit, level
                    return out
            raise RuntimeError(f"sample_joint: R + j I has a non-positive pivot at every one of the {self.maxjitter} jitter levels, "
                               "the residual covariance is unstable")

    # ---- the greedy choice of a non-redundant batch of rows (csrc/select_batch.h) -----------------------
    def select_batch(self, xs: torch.Tensor, count: int, noise: float, given: Optional[torch.Tensor] = None, return_variance: bool = False):
        """The ``count`` rows of ``xs`` a greedy maximisation of I(A) = 1/2 sum_k log det(I + C_k[A, A] / noise) picks (gdrf_select_batch,
        csrc/select_batch.h has the definition), C_k the covariances of predict_cov: (indices (count,) int64 in the order picked, gains
        (count,) float64[, variance (K, n) float64: the conditional variances after the last pick]).  ``given`` (G, D): rows already
        sampled, conditioned on first.  All rows at once: n + G <= n_cap and G + count <= SELECT_MAX_PICKS.  No n x n matrix is formed.
        Same jitter-level protocol for K_uu as predict()."""
        count, noise, G = check_select_args(count, noise, int(xs.shape[0]), given, int(xs.shape[1]) if xs.dim() == 2 else None)
        if noise is None:
            raise ValueError("noise must be a positive finite number, got None")
        self._chk_rows(xs)
        n = xs.shape[0]
        if G:
            self._chk_rows(given)
        if n + G > self.n_cap:
            raise ValueError(f"select_batch needs n + G <= n_cap ({n} + {G} > {self.n_cap})")
        self.refresh_inducing()

        def run():
            idx = torch.empty(count, dtype=torch.int64, device=self.device)
            gains = torch.empty(count, dtype=torch.float64, device=self.device)
            var = torch.empty(self.K, n, dtype=torch.float64, device=self.device) if return_variance else None
            _lib.check(self.lib.gdrf_select_batch(self.ctx, xs.data_ptr(), n, self.Z.data_ptr(), self.params.data_ptr(),
                                                  given.data_ptr() if G else None, G, count, noise, idx.data_ptr(), gains.data_ptr(),
                                                  var.data_ptr() if var is not None else None, _stream_ptr(self.device)), "gdrf_select_batch")
            return (idx, gains, var) if return_variance else (idx, gains)

        return self._speculated(run)

    # ---- the greedy conditional-variance choice of inducing points (csrc/select_inducing.h) ----------------
    def select_inducing(self, xs: torch.Tensor, count: int, given: Optional[torch.Tensor] = None, floor: float = 0.0,
                        return_residual: bool = False):
        """The ``count`` rows of ``xs`` the pivoted partial Cholesky of the prior kernel matrix K_nn picks (gdrf_select_inducing,
        csrc/select_inducing.h has the definition), at the kernel hyper-parameters in ``params``: (indices (count,) int64 in the order
        picked, pivots (G + count,) float64, residual trace tr(K_nn - Q_nn) after every pick (G + count,) float64, rank[, residual (n,)
        float64: diag(K_nn - Q_nn) after the last pick]).  ``given`` (G, D): points already there, forced pivots ahead of the free picks;
        ``count`` = 0 scores them.  A pivot at or below ``floor`` is degenerate and does not count towards the rank.  All rows at once:
        n + G <= n_cap and G + count <= INDUCING_MAX_PICKS.  No factorisation is needed and neither Z nor the variational parameters
        enter; the (G + count + 1) (n + G) solve-precision elements it needs are held for the call only."""
        count, floor, G = check_inducing_args(count, floor, int(xs.shape[0]), given, int(xs.shape[1]) if xs.dim() == 2 else None)
        if floor is None:
            raise ValueError("floor must be a finite number >= 0, got None")
        self._chk_rows(xs)
        n = xs.shape[0]
        if G:
            self._chk_rows(given)
        if n + G > self.n_cap:
            raise ValueError(f"select_inducing needs n + G <= n_cap ({n} + {G} > {self.n_cap})")
        idx = torch.empty(count, dtype=torch.int64, device=self.device)
        pivots = torch.empty(G + count, dtype=torch.float64, device=self.device)
        trace = torch.empty(G + count, dtype=torch.float64, device=self.device)
        resid = torch.empty(n, dtype=torch.float64, device=self.device) if return_residual else None
        rank = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gdrf_select_inducing(self.ctx, xs.data_ptr(), n, self.params.data_ptr(), given.data_ptr() if G else None, G, count,
                                                 floor, idx.data_ptr() if count else None, pivots.data_ptr(), trace.data_ptr(),
                                                 resid.data_ptr() if resid is not None else None, rank.data_ptr(), _stream_ptr(self.device)),
                   "gdrf_select_inducing")
        rank = int(rank.item())
        return (idx, pivots, trace, rank, resid) if return_residual else (idx, pivots, trace, rank)
