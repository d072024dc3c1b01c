"""``SparseMultinomialGDRF`` with the reference's constructor, predictive and bookkeeping surface
(gdrf/models/sparse_gdrf.py:16-123,161-190,321-409; gdrf/models/abstract_gdrf.py:26-139;
gdrf/models/topic_model.py:148-202), evaluated by hand-written HIP kernels.

Host side keeps only shapes, bounds and the flat parameter vector (a PyTorch-ROCm tensor used as
storage); all arithmetic of model/guide/log_topic_probs runs in libgdrf_hip.  ``model`` and
``guide`` are handles for :class:`gdrf_amd.infer.SVI` exactly as ``pyro.infer.SVI(model=model.model,
guide=model.guide, ...)`` takes them (gdrf/train_script.py:365-371).
"""
from __future__ import annotations

import copy
import functools
import math
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch

from ..data import check_counts, csr_rows, csr_to, is_sparse_counts
from ..engine import (INFO_NAMES, LOO_NAMES, QUANT_DOMINANT, QUANT_EXCEED, QUANT_QUANTILE, SCORE_NAMES, Engine, check_count_args, check_fold_args,
                      check_loo_args, check_psis_args,
                      check_joint_args, check_mc_args, check_quant_args, check_score_args, check_select_args, check_inducing_args, thin_rows)
from ..kernels import Kernel, Product, embedded_coordinates

# The most rows choose_inducing_points looks at by default (more are thinned), and inducing_init="greedy" always
GREEDY_MAX_CANDIDATES = 131072

_PARAM_KEYS = {  # state_dict names follow pyro's "<name>_unconstrained" convention
    "log_lengthscale": "_kernel.lengthscale_unconstrained",
    "log_variance": "_kernel.variance_unconstrained",
    "log_noise": "noise_unconstrained",
    "u_loc": "u_loc_unconstrained",
    "phi_unc": "_word_topic_matrix_map_unconstrained",
    "u_scale_tril_unc": "u_scale_tril_unconstrained",
    "inducing_unc": "_inducing_points_unconstrained",          # only when fixed_inducing_points=False
    "log_scale_mixture": "_kernel.scale_mixture_unconstrained",  # only with the RationalQuadratic kernel
    "log_period": "_kernel.period_unconstrained",                # only with the Periodic kernel
}
_FACTOR_KEYS = {"log_variance": "variance", "log_lengthscale": "lengthscale", "log_period": "period"}



def state_key(name: str) -> str:
    """The state-dict name of an engine parameter: pyro's module path plus "_unconstrained".  A product factor's parameters
    ("kern0.log_variance", "kern0.kern1.log_period") become "_kernel.kern0.variance_unconstrained", ..."""
    if name in _PARAM_KEYS:
        return _PARAM_KEYS[name]
    path, _, leaf = name.rpartition(".")
    if path.startswith("kern") and leaf in _FACTOR_KEYS:
        return f"_kernel.{path}.{_FACTOR_KEYS[leaf]}_unconstrained"
    return name


def product_table(kernel: Kernel, n_dims: int):
    """The factor table a kernel runs with on a product context (Engine(kernel="product", product=...)), or None when it runs as its own
    kind: a Product, or a lone RBF / Periodic whose explicit active_dims are not all of the world's axes (a one-factor product)."""
    lone_subset = kernel.subset_dims and kernel.explicit_active_dims and kernel.active_dims != list(range(n_dims))
    if kernel.name != Product.name and not lone_subset:
        return None
    return [dict(name=path, kind=k.name, active_dims=list(k.active_dims), lengthscales=k.lengthscale.numel(),
                 periods=k.period.numel() if "period" in k.params else 0) for path, k in kernel.factors()]


def kernel_spec(kernel: Kernel) -> dict:
    """The structure of a kernel as plain values (a checkpoint's meta): kinds, active_dims and parameter counts, no values."""
    if kernel.name == Product.name:
        return dict(kind="product", kern0=kernel_spec(kernel.kern0), kern1=kernel_spec(kernel.kern1))
    spec = dict(kind=kernel.name, input_dim=kernel.input_dim, lengthscales=kernel.lengthscale.numel(),
                active_dims=list(kernel.active_dims) if kernel.explicit_active_dims else None)
    if "period" in kernel.params:
        spec["periods"] = kernel.period.numel()
    return spec


def kernel_from_spec(spec: dict) -> Kernel:
    """A kernel of the structure ``spec`` (kernel_spec) with placeholder values of the right shapes (load_state_dict fills them)."""
    from ..kernels import KERNEL_DICT, Periodic
    if spec["kind"] == "product":
        return Product(kernel_from_spec(spec["kern0"]), kernel_from_spec(spec["kern1"]))
    n, nl = int(spec["input_dim"]), int(spec["lengthscales"])
    kw = dict(input_dim=n, lengthscale=torch.ones(nl) if nl > 1 else 1.0, variance=1.0, active_dims=spec.get("active_dims"))
    if spec["kind"] == Periodic.name:
        npr = int(spec["periods"])
        return Periodic(period=torch.ones(npr) if npr > 1 else 1.0, **kw)
    return KERNEL_DICT[spec["kind"]](**kw)


def legacy_kernel_spec(meta: dict, state: Dict[str, torch.Tensor]) -> dict:
    """The kernel_spec of a checkpoint written before every snapshot carried one (``meta["kernel_spec"]`` absent or None): a lone kernel
    over all D axes, ARD or per-axis periods exactly when the stored log-lengthscales or log-periods are (D,) vectors."""
    D = int(meta["D"])
    count = lambda name: D if state[_PARAM_KEYS[name]].dim() == 1 else 1
    spec = dict(kind=meta["kernel"], input_dim=D, lengthscales=count("log_lengthscale"), active_dims=None)
    if _PARAM_KEYS["log_period"] in state:
        spec["periods"] = count("log_period")
    return spec


MEAN_PREFIX = "_mean_function."      # + the name from named_parameters(): a trainable parameter of a torch.nn.Module mean_function


def learnable_mean_parameters(mean_function) -> List[Tuple[str, torch.nn.Parameter]]:
    """The parameters of a mean_function that SVI.step trains, as (state_dict name, parameter): those of a ``torch.nn.Module`` whose
    ``requires_grad`` is set.  In the reference the mean_function is an attribute of a gp.Parameterized (abstract_gdrf.py:33-48), so
    pyro.module puts a Module's parameters into the param store and SVI.step updates them; frozen ones get no gradient and stay.  Plain
    callables, None and modules without trainable parameters give [] (their values are data to the step)."""
    if not isinstance(mean_function, torch.nn.Module):
        return []
    return [(MEAN_PREFIX + n, p) for n, p in mean_function.named_parameters() if p.requires_grad]


def validate_dirichlet_param(b: torch.Tensor, K: int, V: int) -> torch.Tensor:
    """gdrf/models/utils.py:6-24."""
    b = torch.as_tensor(b, dtype=torch.float64)
    assert (b <= 0).sum().item() == 0, "b must be positive"
    if b.dim() == 0:
        return torch.ones(K, V, dtype=torch.float64) * b
    if b.dim() == 1:
        if b.shape[0] == K:
            return b.repeat(V, 1).T.contiguous()
        if b.shape[0] == V:
            return b.repeat(K, 1)
        raise ValueError("parameter b must have length K or V if 1D")
    if b.dim() == 2:
        assert tuple(b.shape) == (K, V), "b should be KxV if 2D"
        return b
    raise ValueError("invalid b parameter- you passed %s" % (b,))


# Rows one Monte-Carlo predictive call holds in the engine: like forward(), the call grows the engine to hold its rows, but only up to
# this many (the engine's workspaces take about 3 M elements per row); more rows are cut into pieces of the engine's n_cap.
MC_PIECE_ROWS = 65536


def row_pieces(n: int, size: int):
    """The rows [0, n) in pieces of at most ``size``: (a, b, whole) of each piece [a, b), ``whole`` when it is all the rows"""
    for a in range(0, n, size):
        b = min(n, a + size)
        yield a, b, (a, b) == (0, n)


def count_rows(w, a: int, b: int, whole: bool = False):
    """Rows [a, b) of dense or CSR counts.  None stays None; a ``whole`` piece is the caller's object itself, which keeps the engine's
    per-tensor caches."""
    if w is None or whole:
        return w
    return csr_rows(w, slice(a, b)) if is_sparse_counts(w) else w[a:b]


def join_pieces(parts: list, axis):
    """The results of the pieces as one: joined along ``axis`` (a single part as it is), added when ``axis`` is None.  A tuple of axes
    joins parts that are tuples, element by element."""
    if isinstance(axis, tuple):
        return tuple(join_pieces([p[i] for p in parts], ax) for i, ax in enumerate(axis))
    if axis is None:
        return torch.stack(parts).sum(0)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=axis)


class ModelSnapshot:
    """What ``deepcopy(model).half()`` yields for checkpoints (gdrf/train_script.py:490-506): a detached copy of the parameters
    that supports ``.half()/.float()/.state_dict()`` AND the read-only model surface the end-of-run artefact writer uses on a
    loaded checkpoint (gdrf/utils/loggers.py:35-47: ``torch.load(ckpt)["model"]`` then ``.dims``, ``.K``, ``.topic_probs(xs)``,
    ``.word_probs(xs)``, ``.word_topic_matrix``).

    It holds tensors and plain Python values only (``meta``: sizes, world, kernel name, inducing inputs, Dirichlet parameter,
    jitter schedule): ``torch.save`` / ``torch.load(..., weights_only=True)`` round-trip it once the class is allow-listed
    (``torch.serialization.add_safe_globals([ModelSnapshot])``), and ``to_payload()`` / ``from_payload()`` give the same content
    as a plain dict for loaders that allow no classes at all.  The predictive methods rebuild a device model lazily
    (``restore()``); a ``mean_function`` / ``link_function`` callable is not part of a checkpoint (the reference pickles them by
    reference only) - pass them to ``restore()`` when the run used them."""

    def __init__(self, state: Dict[str, torch.Tensor], meta: dict):
        self._state = state
        self.meta = meta
        self._model = None

    # ---- pickling: tensors and primitives only (the lazily rebuilt device model never travels)
    def __getstate__(self):
        return {"_state": self._state, "meta": self.meta}

    def __setstate__(self, d):
        self._state, self.meta, self._model = d["_state"], d["meta"], None

    def to_payload(self) -> dict:
        return {"state": dict(self._state), "meta": dict(self.meta)}

    @classmethod
    def from_payload(cls, payload: dict) -> "ModelSnapshot":
        return cls(dict(payload["state"]), dict(payload["meta"]))

    def half(self):
        return ModelSnapshot({k: v.half() for k, v in self._state.items()}, self.meta)

    def float(self):
        return ModelSnapshot({k: v.float() for k, v in self._state.items()}, self.meta)

    def state_dict(self):
        return dict(self._state)

    def parameters(self):
        return list(self._state.values())

    # ---- the model surface of gdrf/models/abstract_gdrf.py:86-139 that needs no device
    @property
    def dims(self) -> int:
        return int(self.meta["D"])

    @property
    def K(self) -> int:
        return int(self.meta["K"])

    @property
    def V(self) -> int:
        return int(self.meta["V"])

    @property
    def word_topic_matrix(self) -> torch.Tensor:
        return torch.softmax(self._state[_PARAM_KEYS["phi_unc"]].float(), dim=-1)

    # ---- the part that does: a device model with these parameters, built on first use
    def restore(self, device: Optional[str] = None, mean_function: Callable = None, link_function: Callable = None):
        """A ``SparseMultinomialGDRF`` on ``device`` (default: the device the snapshot was taken on) holding these parameters.  A
        ``torch.nn.Module`` mean_function receives the stored ``_mean_function.*`` values; without one those entries are not used."""
        m = self.meta
        if self._model is not None and device is None and mean_function is None and link_function is None:
            return self._model
        kern = kernel_from_spec(m.get("kernel_spec") or legacy_kernel_spec(m, self._state))
        dtype = getattr(torch, m["dtype"])
        model = SparseMultinomialGDRF(
            num_observation_categories=int(m["V"]), num_topic_categories=int(m["K"]), world=[tuple(w) for w in m["world"]],
            kernel=kern, dirichlet_param=torch.as_tensor(m["dirichlet_param"]), n_points=list(m["n_points"]),
            fixed_inducing_points=bool(m["fixed_inducing_points"]), inducing_points=torch.as_tensor(m["inducing_points"]),
            mean_function=mean_function, link_function=link_function, noise=1.0, device=device or m["device"],
            whiten=bool(m["whiten"]), jitter=float(m["jitter"]), maxjitter=int(m["maxjitter"]), dtype=dtype,
            pure_fp32=bool(m["pure_fp32"]), mfma_mode=m["mfma_mode"], seed=int(m["seed"]), guide_rescale=bool(m["guide_rescale"]),
            rows_form=m.get("rows_form", "auto"))
        keys = {state_key(n) for n in model._param_names()}
        model.load_state_dict({k: v.to(dtype) for k, v in self._state.items() if k in keys or not k.startswith(MEAN_PREFIX)})
        if device is None and mean_function is None and link_function is None:
            self._model = model
        return model

    # the predictive methods (SNAPSHOT_METHODS, installed below the model they forward to) all go through restore()


# var_log_lik above which a row's WAIC term is held to be unreliable (Vehtari, Gelman & Gabry 2017, section 2.2)
WAIC_HIGH_VARIANCE = 0.4


def waic_from_pointwise(d: Dict[str, torch.Tensor]) -> Dict[str, object]:
    """WAIC from the (N,) maps of pointwise_log_likelihood (``lpd`` and ``var_log_lik`` are read), in float64 torch on whatever device
    they live on: ``pointwise`` elpd_n = lpd_n - var_log_lik_n, ``elpd_waic`` its sum, ``p_waic`` = sum_n var_log_lik_n (the effective
    number of parameters), ``waic`` = -2 elpd_waic, ``se`` = sqrt(N var(elpd_n)) with the unbiased variance over the rows (0 for
    N = 1), and ``n_high_variance`` the rows with var_log_lik > WAIC_HIGH_VARIANCE."""
    lpd, var = torch.as_tensor(d["lpd"]).double(), torch.as_tensor(d["var_log_lik"]).double()
    if lpd.dim() != 1 or lpd.shape != var.shape or lpd.numel() < 1:
        raise ValueError(f"lpd and var_log_lik must be (N,) maps of the same N >= 1, got {tuple(lpd.shape)} and {tuple(var.shape)}")
    point = lpd - var
    N = point.numel()
    elpd = point.sum()
    se = torch.sqrt(N * point.var(unbiased=True)) if N > 1 else torch.zeros((), dtype=torch.float64, device=point.device)
    return dict(elpd_waic=elpd, p_waic=var.sum(), waic=-2.0 * elpd, se=se, pointwise=point, n_high_variance=int((var > WAIC_HIGH_VARIANCE).sum()))


def _sum_and_se(point: torch.Tensor):
    """(sum, sqrt(N var)) of the (N,) pointwise terms, the unbiased variance over the rows, 0 for N = 1 - as waic_from_pointwise forms its own"""
    N = point.numel()
    se = torch.sqrt(N * point.var(unbiased=True)) if N > 1 else torch.zeros((), dtype=torch.float64, device=point.device)
    return point.sum(), se


def loo_from_pointwise(d: Dict[str, torch.Tensor], num_samples: Optional[int] = None) -> Dict[str, object]:
    """PSIS leave-one-out from the (N,) maps of pointwise_loo (``elpd_loo``, ``lpd``, ``pareto_k`` and ``ess`` are read), in float64 torch
    on whatever device they live on: ``elpd_loo`` the sum of the pointwise terms, ``p_loo`` = sum_n (lpd_n - elpd_loo_n) (the effective
    number of parameters), ``looic`` = -2 elpd_loo, ``se`` = sqrt(N var(elpd_loo_n)) with the unbiased variance over the rows (0 for
    N = 1), the ``pointwise`` terms, ``pareto_k`` and ``ess`` as they came, ``k_threshold`` = min(1 - 1 / log10(S), 0.7) (Vehtari et al.
    2024) with S = ``num_samples`` or, without it, d["num_samples"] or the rows of d["log_lik"], ``n_bad_k`` the rows with pareto_k above
    the threshold (there the estimate is unreliable; NaN does not count) and ``n_not_fitted`` the rows whose pareto_k is NaN (constant
    log likelihoods or an underflowing tail: nothing was smoothed)."""
    point, lpd, k = (torch.as_tensor(d[name]).double() for name in ("elpd_loo", "lpd", "pareto_k"))
    if point.dim() != 1 or point.numel() < 1 or lpd.shape != point.shape or k.shape != point.shape:
        raise ValueError(f"elpd_loo, lpd and pareto_k must be (N,) maps of the same N >= 1, got {tuple(point.shape)}, {tuple(lpd.shape)} and {tuple(k.shape)}")
    if num_samples is None:
        num_samples = d["num_samples"] if "num_samples" in d else d["log_lik"].shape[0] if "log_lik" in d else None
    if num_samples is None or int(num_samples) < 2:
        raise ValueError("loo_from_pointwise needs num_samples >= 2 (as an argument, as d['num_samples'] or through d['log_lik'])")
    elpd, se = _sum_and_se(point)
    thr = min(1.0 - 1.0 / math.log10(int(num_samples)), 0.7)
    return dict(elpd_loo=elpd, p_loo=(lpd - point).sum(), looic=-2.0 * elpd, se=se, pointwise=point, pareto_k=k, ess=torch.as_tensor(d["ess"]).double(),
                k_threshold=thr, n_bad_k=int((k > thr).sum()), n_not_fitted=int(torch.isnan(k).sum()))


def compare_pointwise(a, b) -> Dict[str, torch.Tensor]:
    """Two fits on the same rows from their (N,) pointwise terms, of WAIC or of LOO (the ``pointwise`` entries): ``elpd_diff`` = sum(a - b),
    positive where the first fit predicts better, and ``se_diff`` = sqrt(N var(a - b)), the standard error of that difference (the
    unbiased variance over the rows, 0 for N = 1) - far smaller than the two standard errors suggest, because the rows are paired."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    if a.dim() != 1 or a.shape != b.shape or a.numel() < 1:
        raise ValueError(f"the pointwise terms must be (N,) vectors over the same N >= 1 rows, got {tuple(a.shape)} and {tuple(b.shape)}")
    diff, se = _sum_and_se(a - b)
    return dict(elpd_diff=diff, se_diff=se)


def _all_words(V: int, words):
    """the word list of a call: None is every word"""
    return torch.arange(V, dtype=torch.int32) if words is None else words


def _predict_quant(model, name: str, xs, mode: int, levels, words, num_samples, seed, eps) -> torch.Tensor:
    """What topic_probs_quantiles, word_probs_quantiles, exceedance and dominant_topic_probs share: the link refusal, the argument checks
    (before the device is touched), the word list as the device takes it, and Engine.predict_quant over pieces of at most the engine's
    n_cap rows (_mc_pieces), joined along the row axis: axis 1, axis 0 for the dominant-topic mode."""
    if model._link_function is not None:
        raise NotImplementedError(f"{name} with a custom link_function: the kernel fuses the softmax link")
    n = int(torch.as_tensor(xs).shape[0])
    S, lv, nw = check_quant_args(mode, num_samples, model._K, model._V, n, levels, words, eps)
    xs_s, _ = model._prepare_inputs(xs)
    w = torch.as_tensor(words).to(device=model.device, dtype=torch.int32).contiguous() if nw else None
    return model._mc_pieces(xs_s, lambda eng, x, *_, **kw: eng.predict_quant(x, mode, S, levels=lv if lv else None, words=w, **kw),
                            0 if mode == QUANT_DOMINANT else 1, seed, eps)


class SparseMultinomialGDRF:
    def __init__(
        self,
        num_observation_categories: int,
        num_topic_categories: int,
        world: List[Tuple[float, float]],
        kernel: Kernel,
        dirichlet_param: Union[float, torch.Tensor],
        n_points: Union[int, List[int]],
        fixed_inducing_points: bool = False,
        inducing_init: str = "random",
        mean_function: Callable = None,
        link_function: Callable = None,
        noise: Optional[float] = None,
        device: str = "cuda:0",
        whiten: bool = True,
        jitter: float = 1e-8,
        maxjitter: int = 5,
        randomize_wt_matrix: bool = False,
        randomize_metric=None,
        randomize_iters: int = 100,
        dtype: torch.dtype = torch.float32,
        pure_fp32: bool = False,
        mfma_mode: str = "auto",
        hyper_backward: str = "auto",
        rows_form: str = "auto",
        inducing_points: Optional[torch.Tensor] = None,
        seed: Optional[int] = None,
        guide_rescale: bool = True,
        inducing_candidates: Optional[torch.Tensor] = None,
        **kwargs,
    ):
        """``inducing_init``: "random" and "grid" are the reference's tensor-product meshes over the world.  "greedy" chooses the M =
        prod(n_points) inducing points among rows of the data, by the conditional-variance rule of choose_inducing_points at the kernel's
        initial hyper-parameters; the candidates are ``inducing_candidates`` (N, D) or, without them, the ``xs`` handed to the constructor
        (more than 131072 rows are thinned as choose_inducing_points thins them).  It raises a ValueError where the data hold fewer than M
        distinct places under this kernel.  The ranks of a multi-GPU run do not talk in the constructor: hand every rank the same
        candidates (not its own shard of the rows), or the ranks start from different inducing points.  An explicit ``inducing_points``
        tensor takes precedence over ``inducing_init`` (deep copies, snapshots and engine growth pass the stored points: nothing is
        selected again)."""
        if link_function is not None and not callable(link_function):
            raise TypeError("link_function must be callable")
        # abstract_gdrf.py:34-50: None = softmax over the topics (fused into the row kernel).  A callable maps the (K, N) tensor mu to
        # (K, N) topic weights; the step then evaluates it (and its Jacobian, by autograd) with torch between three library calls
        # (gdrf_step_local_link), and the predictive methods apply it to log_topic_probs as abstract_gdrf.py:113-119,137-139 do.
        self._link_function = link_function
        if mean_function is not None and not callable(mean_function):
            raise TypeError("mean_function must be callable")
        if randomize_metric is not None and not callable(randomize_metric):
            raise TypeError("randomize_metric must be callable")
        # abstract_gdrf.py:38-48: evaluated on the scaled inputs every step; its values are data to the fused step.  The trainable
        # parameters of a torch.nn.Module mean (learnable_mean_parameters) are one more segment of the engine's parameter vector: the
        # step chains the row adjoints of the mean values through the module by autograd (_step_means) and the optimizer updates them
        # with the rest; after every step the module holds the engine's values (_mean_to_module)
        self._mean_function = mean_function
        self._mean_params = learnable_mean_parameters(mean_function)
        self._mean_versions = None
        # quirk Q3 (sparse_gdrf.py:376-380): the reference's guide scales its inputs twice.  True reproduces that (for a world
        # other than the unit cube the step then evaluates the GP predictive at two input sets, gdrf_step_local2); False scales
        # once on both sides.  No effect for the unit-cube world train() builds.
        self._guide_rescale = bool(guide_rescale)
        self._randomize_metric, self._randomize_iters = randomize_metric, int(randomize_iters)
        if not isinstance(kernel, Kernel):
            raise TypeError("kernel must be a gdrf_amd.kernels.RBF or Matern52")
        self._product = product_table(kernel, len(world))
        if self._product is None and kernel.name == "periodic" and kernel.input_dim > 2:
            raise ValueError(f"the Periodic kernel supports at most 2 input dimensions, got input_dim = {kernel.input_dim}")
        if self._product is not None:
            bad = [d for d in kernel.active_dims if d >= len(world)]
            if bad:
                raise ValueError(f"kernel active_dims {bad} are not axes of the {len(world)}-dimensional world")
            if embedded_coordinates(kernel) > 4:
                raise ValueError(f"the kernel needs {embedded_coordinates(kernel)} embedded coordinates (one per RBF axis, two per Periodic "
                                 "axis); at most 4 are supported")
        self._V = int(num_observation_categories)
        self._K = int(num_topic_categories)
        self._world = [(float(a), float(b)) for a, b in world]
        self._n_dims = len(self._world)
        self.device = torch.device(device)
        for name, p in self._mean_params:
            if p.device.type != self.device.type or (self.device.index is not None and p.device.index != self.device.index):
                raise ValueError(f"mean_function parameter {name[len(MEAN_PREFIX):]!r} is on {p.device}, the model on {self.device}: "
                                 "move the module to the model's device")
        self.dtype = dtype
        self._pure_fp32 = bool(pure_fp32)
        self._mfma_mode = mfma_mode          # Engine(mfma_mode=...): "auto" | "f32" | "bf16x6" | "f16x3"
        self._hyper_backward = hyper_backward   # Engine(hyper_backward=...): "auto" | "tn" | "f64" (csrc/hyper_tn.h)
        if rows_form not in ("auto", "streamed"):
            raise ValueError("rows_form must be 'auto' or 'streamed'")
        self._rows_form = rows_form          # Engine(rows_form=...): "auto" (LDS row forms) | "streamed" (any V, csrc/rows_vstream.h)
        self._kernel = kernel
        if self._product is None and kernel.input_dim != self._n_dims:
            raise ValueError("kernel.input_dim does not match the world's dimensionality")
        self._lower = torch.tensor([b[0] for b in self._world], dtype=torch.float64)
        self._upper = torch.tensor([b[1] for b in self._world], dtype=torch.float64)
        self._delta = self._upper - self._lower
        self._jitter, self._maxjitter, self._whiten = float(jitter), int(maxjitter), bool(whiten)
        self._fixed_inducing_points = bool(fixed_inducing_points)   # False: Z is an interval(0,1)-constrained parameter
        if isinstance(dirichlet_param, float):
            dirichlet_param = torch.tensor(dirichlet_param)
        self._dirichlet_param = validate_dirichlet_param(dirichlet_param, self._K, self._V)
        self._n_points = [n_points for _ in self._world] if isinstance(n_points, int) else list(n_points)
        self.rng_seed = int(torch.initial_seed() if seed is None else seed) & (2 ** 63 - 1)
        gen = torch.Generator().manual_seed(self.rng_seed)
        # ---- inducing points: sparse_gdrf.py:54-77
        greedy_candidates = None
        if inducing_points is not None:
            Z = torch.as_tensor(inducing_points, dtype=torch.float64)
        else:
            if inducing_init == "random":
                pts = [torch.sort(torch.rand(self._n_points[i], generator=gen, dtype=torch.float64))[0] * self._delta[i]
                       + self._lower[i] for i in range(self._n_dims)]
            elif inducing_init == "grid":
                pts = [torch.arange(b[0], b[1] + (b[1] - b[0]) / (n - 1) - 1e-10, (b[1] - b[0]) / (n - 1), dtype=torch.float64)
                       for b, n in zip(self._world, self._n_points)]
            elif inducing_init == "greedy":
                pts = None
            else:
                raise ValueError(f"inducing_init argument {inducing_init} not valid. Only 'random' and 'grid' are "
                                 "currently supported, and 'greedy' (inducing points chosen among the rows of the data)")
            if pts is None:
                cand = inducing_candidates if inducing_candidates is not None else kwargs.get("xs")
                if cand is None:
                    raise ValueError("inducing_init='greedy' chooses the inducing points among rows of the data: pass xs= or "
                                     "inducing_candidates= to the constructor")
                cand = torch.as_tensor(cand)
                if cand.dim() == 1 and self._n_dims == 1:
                    cand = cand.unsqueeze(-1)
                M_greedy = math.prod(int(n) for n in self._n_points)
                if cand.dim() != 2 or cand.shape[1] != self._n_dims:
                    raise ValueError(f"the candidates of inducing_init='greedy' must have shape (N, {self._n_dims}), got {tuple(cand.shape)}")
                check_inducing_args(M_greedy, None, min(int(cand.shape[0]), GREEDY_MAX_CANDIDATES))
                greedy_candidates = cand
                Z = torch.zeros(M_greedy, self._n_dims, dtype=torch.float64)       # a placeholder until _init_params has chosen
            else:
                Z = torch.stack([x.flatten() for x in torch.meshgrid(*pts, indexing="ij")]).T
                Z = (Z - self._lower) / self._delta
        self._greedy_candidates = greedy_candidates
        self._inducing_points = Z.to(dtype).contiguous()
        self.M, self.D = int(Z.shape[0]), int(Z.shape[1])
        self.latent_shape = torch.Size([self._K])
        self._engine: Optional[Engine] = None
        self._init_noise = 1.0 if noise is None else float(noise)
        self._randomize_wt = bool(randomize_wt_matrix)
        self._gen = gen
        xs = kwargs.get("xs")
        ws0 = kwargs.get("ws")
        if ws0 is not None and is_sparse_counts(ws0):      # a sparse count matrix: validated here, before the device is touched
            check_counts(ws0, int(xs.shape[0]) if xs is not None else None, self._V)
        n0 = int(xs.shape[0]) if xs is not None else 1
        if greedy_candidates is not None:              # the engine that chooses holds the (thinned) candidates
            n0 = max(n0, min(int(greedy_candidates.shape[0]), GREEDY_MAX_CANDIDATES))
        self._engine_for(n0)

    # ------------------------------------------------------------------ engine / parameters
    def _engine_for(self, n: int) -> Engine:
        e = self._engine
        if e is not None and n <= e.n_cap:
            return e
        new = Engine(n, self.M, self._K, self._V, self.D, dtype=self.dtype, kernel="product" if self._product else self._kernel.name,
                     device=self.device, product=self._product,
                     jitter=self._jitter, maxjitter=self._maxjitter, pure_fp32=self._pure_fp32, mfma_mode=self._mfma_mode,
                     learn_inducing=not self._fixed_inducing_points, whiten=self._whiten, hyper_backward=self._hyper_backward,
                     ard=self._kernel.ard and not self._product, mean_params={n: tuple(p.shape) for n, p in self._mean_params},
                     rows_form=self._rows_form,
                     period_count=self._kernel.period.numel() if self._kernel.name == "periodic" and not self._product else 1)
        new.set_inducing_points(self._inducing_points)
        new.set_dirichlet(self._dirichlet_param)
        new.link_function = self._link_function
        if e is None:
            self._engine = new                  # a randomize_metric may already call the model's methods
            self._init_params(new)
        else:                                   # grow the workspaces, keep parameters and optimizer state
            new.params.copy_(e.params); new.exp_avg.copy_(e.exp_avg); new.exp_avg_sq.copy_(e.exp_avg_sq)
            if e.opt_extra is not None:
                new.state_buffer(3).copy_(e.opt_extra)
            new.opt_step = e.opt_step
        self._engine = new
        self._inducing_points = new.Z
        return new

    def _init_params(self, eng: Engine):
        """sparse_gdrf.py:96-122 and abstract_gdrf.py:57-84."""
        with torch.no_grad():
            for path, k in self._kernel.factors():
                for name in k.params:
                    v = eng.view((path + "." if path else "") + "log_" + name)
                    v.copy_(getattr(k, name).log().reshape(v.shape))
            eng.view("log_noise").fill_(float(torch.tensor(self._init_noise, dtype=torch.float64).log()))
            if self._greedy_candidates is not None:
                # inducing_init="greedy": the kernel's hyper-parameters are in place, nothing below has read Z yet
                cand, self._greedy_candidates = self._greedy_candidates, None
                res = self._choose_inducing(eng, cand, self.M, None, GREEDY_MAX_CANDIDATES, False)
                if res["rank"] < self.M:
                    raise ValueError(f"inducing_init='greedy': the candidates hold only {res['rank']} distinct places under this kernel "
                                     f"(the rank of the selection), fewer than the M = {self.M} inducing points asked for: lower n_points "
                                     "or pass more varied candidates")
                eng.set_inducing_points(res["scaled"])
                self._inducing_points = eng.Z
            eng.view("u_loc").zero_()
            ret = torch.softmax(self._dirichlet_param, dim=-2)           # over K (abstract_gdrf.py:68-69)
            if self._randomize_wt:
                # abstract_gdrf.py:70-78.  `best` is the score of the Dirichlet-parameter matrix and is never raised inside the
                # loop, so the LAST candidate that beats it wins (with no metric: one draw, score 0 > best = -1).
                metric = self._randomize_metric
                as_model = lambda t: t.to(device=self.device, dtype=self.dtype)   # what the reference's metric is handed
                best = -1 if metric is None else metric(as_model(ret), self)
                for _ in range(1 if metric is None else self._randomize_iters):
                    possible = torch.softmax(torch.randn(ret.shape, generator=self._gen, dtype=torch.float64), dim=-2)
                    score = 0 if metric is None else metric(as_model(possible), self)
                    if score > best:
                        ret = possible
            eng.view("phi_unc").copy_(ret.log().to(eng.dtype))            # simplex transform inverse
            eng.factorize()                                               # u_scale_tril = jittercholesky(kernel(Z)) x K
            L = eng.workspace("L").to(eng.dtype)
            unc = L.tril(-1) + torch.diag(L.diagonal().log())             # lower_cholesky transform inverse
            eng.view("u_scale_tril_unc").copy_(unc.unsqueeze(0).expand(self._K, -1, -1))
        self._mean_from_module()

    @property
    def inducing_points(self) -> torch.Tensor:
        """(M, D) inducing inputs in the scaled world; the interval(0,1)-constrained value when they are learnable."""
        self._engine.refresh_inducing()
        return self._engine.Z

    @property
    def K(self):
        return self._K

    @property
    def V(self):
        return self._V

    @property
    def dims(self):
        return self._n_dims

    # ------------------------------------------------------------------ scaling (topic_model.py:168-198)
    def scale(self, input: torch.Tensor) -> torch.Tensor:
        return (input - self._lower.to(input)) / self._delta.to(input)

    def _check_bounds(self, input: torch.Tensor, epsilon: float = 1e-8) -> bool:
        lo, hi = self._lower.to(input), self._upper.to(input)
        return input.shape[-1] == self._n_dims and bool(((input - lo > -epsilon) & (input - hi < epsilon)).all())

    def _guide_inputs(self, xs_scaled: torch.Tensor) -> Optional[torch.Tensor]:
        """The inputs the reference's guide ends up evaluating its predictive at: scale(scale(xs)) (quirk Q3); None when that is
        what the model sees too (unit-cube world, or guide_rescale=False)."""
        unit = all(a == 0.0 and b == 1.0 for a, b in self._world)
        if unit or not self._guide_rescale:
            return None
        return self.scale(xs_scaled.double()).to(self.dtype).contiguous()

    def _prepare_inputs(self, xs, ws=None):
        """@scale_decorator semantics: bounds assertion then the affine map to the unit cube (identity for the
        world train() builds, train_script.py:261-271).  The guide's second scaling (quirk Q3): _guide_inputs."""
        xs = torch.as_tensor(xs)
        if xs.dim() == 1:
            xs = xs.unsqueeze(-1)
        xs = xs.to(self.device)
        assert self._check_bounds(xs), "inputs fall outside the model's world bounds"
        unit = all(a == 0.0 and b == 1.0 for a, b in self._world)
        xs_s = xs if unit else self.scale(xs)
        xs_s = xs_s.to(self.dtype).contiguous()
        ws_d = None
        if ws is not None and is_sparse_counts(ws):
            # a torch.sparse_csr count matrix goes through as it is (csrc/rows_csr.h); moving a tensor that already lives on the device
            # returns the same object, so the engine's per-tensor caches hold
            check_counts(ws, xs_s.shape[0], self._V)
            ws_d = csr_to(ws, xs_s.device)
        elif ws is not None:
            ws_d = torch.as_tensor(ws).to(device=self.device, dtype=torch.int32).contiguous()
            if ws_d.shape != (xs_s.shape[0], self._V):
                raise ValueError(f"ws must have shape ({xs_s.shape[0]}, {self._V})")
        return xs_s, ws_d

    def _mean_values(self, xs_scaled: torch.Tensor) -> Optional[torch.Tensor]:
        """mean_function(xs) on the scaled inputs (scale_decorator runs first: sparse_gdrf.py:323-346); None for zero_mean."""
        if self._mean_function is None:
            return None
        with torch.no_grad():
            return torch.as_tensor(self._mean_function(xs_scaled))

    # ------------------------------------------------------------------ trainable mean_function parameters
    def _mean_from_module(self):
        """The module's current parameter values -> the engine's mean segment."""
        with torch.no_grad():
            for name, p in self._mean_params:
                self._engine.view(name).copy_(p.detach())
        self._mean_versions = [p._version for _, p in self._mean_params]

    def _mean_to_module(self):
        """The engine's mean segment (after the optimizer update) -> the module's parameters, in their own dtype."""
        if not self._mean_params:
            return
        with torch.no_grad():
            for name, p in self._mean_params:
                p.copy_(self._engine.view(name))
        self._mean_versions = [p._version for _, p in self._mean_params]

    def _mean_kn(self, values, n: int) -> torch.Tensor:
        """mean_function values on the model's device and in its dtype, expanded to (K, n); ValueError when they do not broadcast."""
        out = torch.as_tensor(values).to(device=self.device, dtype=self.dtype)
        try:
            return out.expand(self._K, n)
        except RuntimeError:
            raise ValueError(f"mean_function returned shape {tuple(out.shape)}, not broadcastable to ({self._K}, {n})") from None

    def _mean_graph(self, xs_scaled: torch.Tensor, n: int) -> torch.Tensor:
        return self._mean_kn(self._mean_function(xs_scaled), n)

    def _step_means(self, xs_scaled: torch.Tensor, xs_guide: Optional[torch.Tensor]):
        """(mean, mean_guide, mean_vjp) of one training step.  Without trainable mean parameters: the values as data, mean_vjp None.
        With them: the values evaluated with grad enabled (model side; guide side too in a non-unit world), passed detached, and the
        vector-Jacobian product that Engine.loss_and_grads calls with the device's row adjoints after every particle - autograd through
        the module, so a broadcast shape's reduction comes from the expand.  The graph is kept for every particle (and a redone step)."""
        if not self._mean_params:
            return self._mean_values(xs_scaled), None if xs_guide is None else self._mean_values(xs_guide), None
        if self._mean_versions != [p._version for _, p in self._mean_params]:
            self._mean_from_module()                 # written outside the step since the last update
        n = xs_scaled.shape[0]
        with torch.enable_grad():
            outs = [self._mean_graph(xs_scaled, n)] + ([] if xs_guide is None else [self._mean_graph(xs_guide, n)])
        params = [p for _, p in self._mean_params]

        def mean_vjp(adj, adj_guide):
            pairs = [(o, a) for o, a in zip(outs, (adj, adj_guide)) if o.requires_grad]
            gs = torch.autograd.grad([o for o, _ in pairs], params, grad_outputs=[a for _, a in pairs], retain_graph=True,
                                     allow_unused=True) if pairs else [None] * len(params)
            return torch.cat([(torch.zeros(p.numel(), dtype=torch.float64, device=self.device) if g is None
                               else g.detach().reshape(-1).to(device=self.device, dtype=torch.float64)) for g, p in zip(gs, params)])
        return outs[0].detach(), None if xs_guide is None else outs[1].detach(), mean_vjp

    # ------------------------------------------------------------------ SVI handles
    def model(self, xs, ws, subsample=False):
        raise NotImplementedError("SparseMultinomialGDRF.model is evaluated through gdrf_amd.infer.SVI (fused with the guide "
                                  "in one HIP forward/backward); it is not a traceable Pyro program")

    def guide(self, xs, ws, subsample=False):
        raise NotImplementedError("SparseMultinomialGDRF.guide is evaluated through gdrf_amd.infer.SVI")

    def train(self, mode: bool = True):
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------ predictive path
    def log_topic_probs(self, xs) -> torch.Tensor:
        """f_loc (K, N): sparse_gdrf.py:161-186 (mean only; the discarded variance is never computed)."""
        xs_s, _ = self._prepare_inputs(xs)
        return self._engine_for(1).predict(xs_s, 0)

    def topic_probs(self, xs) -> torch.Tensor:
        if self._link_function is not None:                  # abstract_gdrf.py:113-115
            return self._link_function(self.log_topic_probs(xs)).T
        xs_s, _ = self._prepare_inputs(xs)
        return self._engine_for(1).predict(xs_s, 1)

    def word_probs(self, xs) -> torch.Tensor:
        if self._link_function is not None:                  # abstract_gdrf.py:117-119
            return self.topic_probs(xs) @ self.word_topic_matrix
        xs_s, _ = self._prepare_inputs(xs)
        return self._engine_for(1).predict(xs_s, 2)

    def forward(self, Xnew, full_cov: bool = False):
        """``SparseGDRF.forward`` (gdrf/models/sparse_gdrf.py:277-319): (loc, var) of the GP posterior q(f(Xnew)), each (K, N) -
        ``gp.util.conditional(Xnew, Z, kernel, u_loc, u_scale_tril, Luu, full_cov=False, whiten=...)`` with the mean_function
        added to loc.  (The reference's own body reads ``self.jitter`` / ``self.maxjitter``, attributes that do not exist - quirk
        Q10 -; this is what it evaluates once those are spelled ``_jitter`` / ``_maxjitter``.)  ``full_cov=True`` would be K dense
        N x N matrices: ``posterior(Xnew)`` returns them."""
        if full_cov:
            raise NotImplementedError("forward(full_cov=True): the K dense N x N posterior covariances are not returned here; "
                                      "posterior(Xnew) returns (loc, cov) with cov of shape (K, N, N)")
        xs_s, _ = self._prepare_inputs(Xnew)
        lv = self._engine_for(xs_s.shape[0]).predict(xs_s, 4)
        loc, var = lv[0], lv[1]
        mean = self._mean_values(xs_s)
        if mean is not None:
            loc = loc + mean.to(loc)
        return loc, var

    __call__ = forward

    def ml_topics(self, xs):
        return torch.argmax(self.log_topic_probs(xs), dim=-2)

    def ml_words(self, xs):
        return torch.argmax(self.word_probs(xs), dim=-2)

    def perplexity(self, x, w) -> torch.Tensor:
        """exp(-sum w log p / sum w): abstract_gdrf.py:137-139, as a 0-d tensor (train_script.py:469-472 calls .item())."""
        if self._link_function is not None:                  # abstract_gdrf.py:137-139, literally
            if is_sparse_counts(w):                          # sum w log p over the stored entries: the counts are never densified
                check_counts(w, None, self._V)
                wd = csr_to(w, self.device)
                crow, val = wd.crow_indices(), wd.values()
                row = torch.repeat_interleave(torch.arange(wd.shape[0], device=self.device), crow[1:] - crow[:-1], output_size=val.numel())
                lp = self.word_probs(x)[row, wd.col_indices().long()].log()
                keep = val != 0                               # a stored zero is an absent entry
                return ((val[keep] * lp[keep]).sum() / -val.sum()).exp()
            wd = torch.as_tensor(w).to(self.device)
            return ((wd * self.word_probs(x).log()).sum() / -wd.sum()).exp()
        xs_s, ws_d = self._prepare_inputs(x, w)
        s = self._engine_for(1).predict(xs_s, 3, ws_d)
        return torch.exp(-s[0] / s[1])

    # ------------------------------------------------------------------ Monte-Carlo predictive path (csrc/predict_mc.h)
    def _mc_pieces(self, xs_s: torch.Tensor, call: Callable, axis, seed=None, eps=None):
        """A predictive engine call on more rows than one call holds: ``call(eng, xs, a, b, whole, seed=, row_offset=, eps=, mean=)`` for
        every piece [a, b) (row_pieces) of at most n_cap rows, on an engine grown to hold min(n, MC_PIECE_ROWS) of them, the results joined
        by join_pieces(axis).  What a call takes is prepared here once - the seed (default: the model's rng_seed), an injected ``eps`` on
        the device, the mean_function's values as (K, n) - and cut to the piece.  The draws are keyed by the global row, row_offset + row,
        so a result does not depend on the piece size."""
        n = xs_s.shape[0]
        eng = self._engine_for(min(n, MC_PIECE_ROWS))
        seed = self.rng_seed if seed is None else int(seed)
        if eps is not None:
            eps = torch.as_tensor(eps).to(device=self.device, dtype=self.dtype)
        mean = self._mean_values(xs_s)
        if mean is not None:
            mean = self._mean_kn(mean, n)
        return join_pieces([call(eng, xs_s[a:b], a, b, whole, seed=seed, row_offset=a, eps=None if eps is None else eps[:, :, a:b].contiguous(),
                                 mean=None if mean is None else mean[:, a:b]) for a, b, whole in row_pieces(n, eng.n_cap)], axis)

    def _predict_mc(self, xs_s: torch.Tensor, mode: int, S: int, ws_d=None, seed=None, eps=None) -> torch.Tensor:
        """Engine.predict_mc over row pieces (_mc_pieces), the dense counts sliced for every piece: the samples of modes 0 and 3 and the
        moments of mode 1 are joined along their row axis, mode 2's two sums are added."""
        return self._mc_pieces(xs_s, lambda eng, x, a, b, whole, **kw: eng.predict_mc(x, mode, S, ws=count_rows(ws_d, a, b), **kw),
                               {0: 1, 1: 1, 2: None, 3: 2}[mode], seed, eps)

    def sample_topic_probs(self, xs, num_samples, seed=None, eps=None) -> torch.Tensor:
        """(S, N, K) samples of the topic proportions under the guide's posterior: theta_s = link(mu_s), mu_s = f_loc + mean + f_var eps_s
        with (f_loc, f_var) = forward(xs) and f_var as the scale, as the guide draws mu (sparse_gdrf.py:403-405).  ``eps``: injected
        (S, K, N) standard normals; otherwise counter-based Philox draws keyed by ``seed`` (default: the model's rng_seed) and
        (row, topic, sample).  topic_probs(xs) is the plug-in softmax(f_loc), which ignores f_var."""
        S = check_mc_args(num_samples, self._K, int(torch.as_tensor(xs).shape[0]), eps)
        xs_s, _ = self._prepare_inputs(xs)
        if self._link_function is not None:      # the link with torch on the raw mu samples, as topic_probs applies it to f_loc
            mu = self._predict_mc(xs_s, 3, S, seed=seed, eps=eps)
            return torch.stack([self._link_function(mu[s]).T for s in range(S)])
        return self._predict_mc(xs_s, 0, S, seed=seed, eps=eps)

    def topic_probs_mc(self, xs, num_samples: int = 256, seed=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean, var), each (N, K): the posterior-predictive topic proportions E_q[link(mu)] and their variance (divisor S) over
        ``num_samples`` draws, reduced on the device without storing the samples."""
        S = check_mc_args(num_samples, self._K, int(torch.as_tensor(xs).shape[0]))
        if self._link_function is not None:
            th = self.sample_topic_probs(xs, S, seed=seed)
            return th.mean(0), th.var(0, unbiased=False)
        xs_s, _ = self._prepare_inputs(xs)
        mv = self._predict_mc(xs_s, 1, S, seed=seed)
        return mv[0], mv[1]

    def word_probs_mc(self, xs, num_samples: int = 256, seed=None) -> torch.Tensor:
        """(N, V) posterior-predictive word distributions: E_q[theta] Phi (the expectation is linear in theta)."""
        check_mc_args(num_samples, self._K, 0)
        return self.topic_probs_mc(xs, num_samples, seed=seed)[0] @ self.word_topic_matrix

    def predictive_perplexity(self, x, w, num_samples: int = 64, seed=None) -> torch.Tensor:
        """exp(-sum_n l_n / sum w), l_n = log (1/S) sum_s prod_v p[s][n][v]^w[n][v]: the Monte-Carlo predictive density of each row's
        counts under q(mu) (the Multinomial coefficient left out, as perplexity leaves it out), as a 0-d tensor."""
        if self._link_function is not None:
            raise NotImplementedError("predictive_perplexity with a custom link_function: the score kernel fuses the softmax link")
        S = check_mc_args(num_samples, self._K, 0, ws=w)
        xs_s, ws_d = self._prepare_inputs(x, w)
        s = self._predict_mc(xs_s, 2, S, ws_d=ws_d, seed=seed)
        return torch.exp(-s[0] / s[1])

    # ------------------------------------------------------------------ per-row predictive densities and WAIC (csrc/predict_score.h)
    def pointwise_log_likelihood(self, xs, ws, num_samples: int = 64, seed=None, eps=None, normalized: bool = False) -> Dict[str, torch.Tensor]:
        """How well the fitted field explains each observed row: a dict of five (N,) float64 tensors over ``num_samples`` draws theta_s of
        sample_topic_probs (the same ``seed`` / ``eps``), with a_s = sum_v w_v log (theta_s Phi)_v: ``lpd`` logsumexp_s(a_s) - log S (the
        l_n that predictive_perplexity sums), ``mean_log_lik`` mean_s a_s, ``var_log_lik`` the unbiased variance of a_s over the draws (0
        for one draw), ``total`` sum_v w_v and ``log_coef`` the log of the row's Multinomial coefficient.  ``lpd`` and ``mean_log_lik``
        leave that coefficient out, as perplexity does; ``normalized=True`` adds it to both.  ``ws``: dense counts or a
        ``torch.sparse_csr`` matrix; no V is too large.  Reduced on the device without storing a sample, over pieces of at most the
        engine's n_cap rows as fold-in cuts them; a row's values do not depend on the pieces."""
        if self._link_function is not None:
            raise NotImplementedError("pointwise_log_likelihood with a custom link_function: the kernel fuses the softmax link")
        n = int(torch.as_tensor(xs).shape[0])
        S = check_score_args(num_samples, self._K, self._V, n, ws, eps)
        xs_s, ws_d = self._prepare_inputs(xs, ws)
        out = self._mc_pieces(xs_s, lambda eng, x, a, b, whole, **kw: eng.predict_score(x, count_rows(ws_d, a, b, whole), S, **kw), 1, seed, eps)
        d = dict(zip(SCORE_NAMES, out))
        if normalized:
            d["lpd"] = d["lpd"] + d["log_coef"]
            d["mean_log_lik"] = d["mean_log_lik"] + d["log_coef"]
        return d

    def waic(self, xs, ws, num_samples: int = 64, seed=None, normalized: bool = False) -> Dict[str, object]:
        """The widely applicable information criterion of the rows (xs, ws) under the guide's posterior, for comparing fits (across K, say):
        waic_from_pointwise of pointwise_log_likelihood - ``elpd_waic`` = sum_n (lpd_n - var_log_lik_n), ``p_waic``, ``waic`` =
        -2 elpd_waic, the standard error ``se`` of elpd_waic over the rows, the ``pointwise`` terms and ``n_high_variance``, the number of
        rows whose var_log_lik is above 0.4 (there WAIC is unreliable).  ``normalized`` as in pointwise_log_likelihood: it shifts every
        model's elpd on the same data by the same constant."""
        return waic_from_pointwise(self.pointwise_log_likelihood(xs, ws, num_samples, seed=seed, normalized=normalized))

    # ------------------------------------------------------------------ PSIS leave-one-out (csrc/predict_loo.h)
    def pointwise_loo(self, xs, ws, num_samples: int = 256, seed=None, eps=None, normalized: bool = False,
                      return_log_lik: bool = False) -> Dict[str, torch.Tensor]:
        """Pareto-smoothed importance-sampling leave-one-out, row by row: a dict of six (N,) float64 tensors from the log likelihoods a_s
        of pointwise_log_likelihood over the same ``num_samples`` draws (``seed`` / ``eps`` as there; 25 .. 1024 draws): ``elpd_loo`` the
        estimate of the row's log predictive density had the row been held out, ``pareto_k`` the shape of the generalised Pareto tail
        fitted to the row's largest importance ratios (above min(1 - 1 / log10(S), 0.7) the estimate is unreliable; NaN where nothing is
        fitted: constant a_s or an underflowing tail), ``ess`` the effective sample size of the smoothed weights, and ``lpd``, ``total``,
        ``log_coef`` as pointwise_log_likelihood returns them, bit for bit.  ``elpd_loo`` and ``lpd`` leave the Multinomial coefficient
        out; ``normalized=True`` adds it to both.  ``return_log_lik=True`` adds ``log_lik``, the (S, N) float64 matrix of the a_s.
        ``ws``: dense counts or a ``torch.sparse_csr`` matrix; no V is too large.  Over pieces of at most the engine's n_cap rows as
        pointwise_log_likelihood cuts them; a row's values do not depend on the pieces.  (A ModelSnapshot does not forward this method:
        call it on ``snap.restore()``.)"""
        if self._link_function is not None:
            raise NotImplementedError("pointwise_loo with a custom link_function: the kernel fuses the softmax link; form the (S, N) log "
                                      "likelihoods with torch and hand them to psis")
        n = int(torch.as_tensor(xs).shape[0])
        S = check_loo_args(num_samples, self._K, self._V, n, ws, eps)
        xs_s, ws_d = self._prepare_inputs(xs, ws)
        call = lambda eng, x, a, b, whole, **kw: eng.predict_loo(x, count_rows(ws_d, a, b, whole), S, return_log_lik=return_log_lik, **kw)
        out = self._mc_pieces(xs_s, call, (1, 1) if return_log_lik else 1, seed, eps)
        d = dict(zip(LOO_NAMES, out[0] if return_log_lik else out))
        if normalized:
            d["elpd_loo"] = d["elpd_loo"] + d["log_coef"]
            d["lpd"] = d["lpd"] + d["log_coef"]
        if return_log_lik:
            d["log_lik"] = out[1]
        return d

    def loo(self, xs, ws, num_samples: int = 256, seed=None, normalized: bool = False) -> Dict[str, object]:
        """PSIS leave-one-out cross-validation of the rows (xs, ws) under the guide's posterior, the remedy where waic reports rows of
        high variance: loo_from_pointwise of pointwise_loo - ``elpd_loo``, ``p_loo``, ``looic`` = -2 elpd_loo, the standard error ``se``,
        the ``pointwise`` terms, ``pareto_k``, ``ess``, ``k_threshold``, ``n_bad_k`` and ``n_not_fitted``.  ``normalized`` as in
        pointwise_loo.  Two fits on the same rows are compared with compare_pointwise of their ``pointwise`` terms.  (A ModelSnapshot does
        not forward this method: call it on ``snap.restore()``.)"""
        return loo_from_pointwise(self.pointwise_loo(xs, ws, num_samples, seed=seed, normalized=normalized), int(num_samples))

    def psis(self, log_lik) -> Dict[str, torch.Tensor]:
        """The PSIS stage on a caller's own (S, n) matrix of log likelihoods - a custom link_function's, or another model's - as a dict of
        the (n,) float64 maps ``elpd_loo``, ``pareto_k`` and ``ess``, over pieces of at most the engine's n_cap columns.  25 <= S <= 1024.
        (A ModelSnapshot does not forward this method: call it on ``snap.restore()``.)"""
        S, n = check_psis_args(torch.as_tensor(log_lik))
        a = torch.as_tensor(log_lik).to(device=self.device, dtype=torch.float64)
        eng = self._engine_for(min(n, MC_PIECE_ROWS))
        out = join_pieces([eng.psis_rows(a[:, lo:hi].contiguous()) for lo, hi, _ in row_pieces(n, eng.n_cap)], 1)
        return dict(zip(LOO_NAMES[:3], out))

    def row_perplexity(self, xs, ws, num_samples: int = 64, seed=None) -> torch.Tensor:
        """(N,) float64: exp(-lpd_n / total_n), the per-token perplexity of each row under the posterior predictive - the map of the samples
        the fitted field explains badly; NaN where a row has no tokens.  predictive_perplexity is the same over all rows at once."""
        d = self.pointwise_log_likelihood(xs, ws, num_samples, seed=seed)
        tot = d["total"]
        return torch.where(tot > 0, torch.exp(-d["lpd"] / tot.clamp_min(1.0)), torch.full_like(tot, float("nan")))

    # ------------------------------------------------------------------ entropy and information-gain maps (csrc/predict_info.h)
    def information(self, xs, num_samples: int = 256, seed=None, eps=None) -> Dict[str, torch.Tensor]:
        """Where the field is still uncertain, and how much of that a sample at x would remove: a dict of six (N,) float64 tensors over
        ``num_samples`` draws theta_s of sample_topic_probs (the same ``seed`` / ``eps``), p_s = theta_s Phi, h(q) = -sum q log q:
        ``topic_entropy`` h(mean_s theta_s), ``topic_expected_entropy`` mean_s h(theta_s), ``topic_information`` their difference, and
        ``word_entropy`` / ``word_expected_entropy`` / ``word_information`` the same for p.  The information values are the Monte-Carlo
        estimates of the mutual information between one token's topic (word) observed at x and the latent field there (BALD); they are
        not clamped, 0 <= word_information <= topic_information <= log min(K, S) up to rounding.  Reduced on the device without storing
        a sample, over pieces of at most the engine's n_cap rows as the other Monte-Carlo calls (_mc_pieces)."""
        if self._link_function is not None:
            raise NotImplementedError("information with a custom link_function: the kernel fuses the softmax link")
        n = int(torch.as_tensor(xs).shape[0])
        S = check_mc_args(num_samples, self._K, n, eps)
        xs_s, _ = self._prepare_inputs(xs)
        return dict(zip(INFO_NAMES, self._mc_pieces(xs_s, lambda eng, x, *_, **kw: eng.predict_info(x, S, **kw), 1, seed, eps)))

    # ------------------------------------------------------------------ credible intervals, exceedance, dominance (csrc/predict_quant.h)
    def topic_probs_quantiles(self, xs, q=(0.05, 0.5, 0.95), num_samples: int = 256, seed=None, eps=None) -> torch.Tensor:
        """(Q, N, K) float64 credible bands of the topic proportions: the type-7 ("linear") sample quantiles at the levels ``q`` in [0, 1]
        (at most QUANT_MAX_LEVELS) of the ``num_samples`` <= QUANT_MAX_SAMPLES draws theta_s of sample_topic_probs (the same ``seed`` /
        ``eps``), ordered on the device without the (S, N, K) samples ever being stored."""
        return _predict_quant(self, "topic_probs_quantiles", xs, QUANT_QUANTILE, q, None, num_samples, seed, eps)

    def word_probs_quantiles(self, xs, q=(0.05, 0.5, 0.95), words=None, num_samples: int = 256, seed=None, eps=None) -> torch.Tensor:
        """(Q, N, W) float64 credible bands of the word probabilities p_s = theta_s Phi at the word indices ``words`` (any order, may
        repeat; None: all V), as topic_probs_quantiles."""
        return _predict_quant(self, "word_probs_quantiles", xs, QUANT_QUANTILE, q, _all_words(self._V, words), num_samples, seed, eps)

    def exceedance(self, xs, thresholds, what: str = "topic", words=None, num_samples: int = 256, seed=None, eps=None) -> torch.Tensor:
        """(Tn, N, C) float64: the share of the ``num_samples`` draws in which the proportion of a topic (``what`` = "topic", C = K) or the
        probability of a word (``what`` = "word", the indices ``words``, None: all V) is strictly above each of the finite
        ``thresholds`` (at most QUANT_MAX_LEVELS; a scalar keeps the leading axis at length 1).  Counted on the device, no sample stored."""
        if what not in ("topic", "word"):
            raise ValueError(f'what must be "topic" or "word", got {what!r}')
        if what == "topic" and words is not None:
            raise ValueError('words goes with what="word"')
        return _predict_quant(self, "exceedance", xs, QUANT_EXCEED, thresholds, _all_words(self._V, words) if what == "word" else None,
                                   num_samples, seed, eps)

    def dominant_topic_probs(self, xs, num_samples: int = 256, seed=None, eps=None) -> torch.Tensor:
        """(N, K) float64: the share of the ``num_samples`` draws in which each topic is the largest one at x (equal values to the
        lower index) - the honest version of ml_topics.  Each row sums to one."""
        return _predict_quant(self, "dominant_topic_probs", xs, QUANT_DOMINANT, None, None, num_samples, seed, eps)

    def most_informative(self, xs, count: int, criterion: str = "word_information", num_samples: int = 256,
                         seed=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(indices, scores) of the ``count`` rows of ``xs`` with the largest ``criterion`` (one of the six names of information()), in
        descending order, equal scores by the lower index.  Each row is ranked on its own: the rows are not chosen to be non-redundant.
        select_batch(xs, count) chooses a non-redundant batch."""
        if criterion not in INFO_NAMES:
            raise ValueError(f"criterion must be one of {INFO_NAMES}, got {criterion!r}")
        n = int(torch.as_tensor(xs).shape[0])
        if isinstance(count, bool) or int(count) != count or not 1 <= int(count) <= n:
            raise ValueError(f"count must be an integer in [1, N = {n}], got {count!r}")
        scores = self.information(xs, num_samples, seed=seed)[criterion]
        order = torch.sort(scores, descending=True, stable=True).indices[:int(count)]
        return order, scores[order]

    # ------------------------------------------------------------------ non-redundant batches of locations (csrc/select_batch.h)
    def select_batch(self, xs, count: int, noise=None, given=None, return_variance: bool = False):
        """Where to take the next ``count`` samples: (indices (count,) int64, gains (count,) float64[, variance (K, N) float64]) of the
        rows of ``xs`` that a greedy maximisation of I(A) = 1/2 sum_k log det(I + C_k[A, A] / s2) picks, in the order picked.  C_k is
        ``posterior(xs)[1][k]`` (never formed here: N is not limited by JOINT_MAX_ROWS), s2 = ``noise`` the variance of the observation
        noise (None: the model's ``noise`` parameter, which governs the independent term between the field and the mu site that a sample's
        tokens inform about).  I(A) is the mutual information between the K latent fields and noisy observations of them at the rows A;
        it is monotone and submodular, so the greedy batch is within (1 - 1/e) of the best one.  gains[t] is what pick t added:
        sum(gains) = I(picked), and the gains never increase.  Equal gains go to the lower index.  ``given`` (G, D): places already
        sampled but not trained on yet; they are conditioned on first, are no candidates and return no gain.  ``return_variance``: the
        variance of every f_k(x_j) given noisy observations at ``given`` and the picks (it starts as ``forward(xs)[1]``).  The link, Phi
        and the mean_function do not enter.  All rows in one call - a greedy choice cannot be cut into row pieces -, G + count <=
        SELECT_MAX_PICKS.  most_informative ranks each row on its own instead."""
        xs_t = torch.as_tensor(xs)
        g_t = None if given is None else torch.as_tensor(given)
        n = int(xs_t.shape[0])
        count, noise, G = check_select_args(count, noise, n, g_t, 1 if xs_t.dim() == 1 else int(xs_t.shape[1]))
        xs_s, _ = self._prepare_inputs(xs_t)
        given_s = self._prepare_inputs(g_t)[0] if G else None
        eng = self._engine_for(n + G)
        if noise is None:
            noise = check_select_args(count, float(self.noise), n)[1]
        return eng.select_batch(xs_s, count, noise, given=given_s, return_variance=return_variance)

    # ------------------------------------------------------------------ inducing points from the data (csrc/select_inducing.h)
    def _kernel_variance_now(self, eng) -> float:
        """k(x, x) at the engine's current hyper-parameters: the variance, a product kernel's product of its factors' variances"""
        names = [n for n in eng.param_names if n == "log_variance" or n.endswith(".log_variance")]
        return math.exp(sum(float(eng.view(n).double().sum()) for n in names))

    def _choose_inducing(self, eng, xs, count, given, max_candidates, return_residual):
        """choose_inducing_points on the engine ``eng`` (the constructor calls it before the model's engine is in place): the argument
        checks, the thinning, the scaling, the floor, Engine.select_inducing and the indices mapped back to the rows of ``xs``"""
        xs_t = torch.as_tensor(xs)
        g_t = None if given is None else torch.as_tensor(given)
        n_all = int(xs_t.shape[0])
        thin = thin_rows(n_all, max_candidates)
        n = n_all if thin is None else int(thin.numel())
        count, _, G = check_inducing_args(count, None, n, g_t, 1 if xs_t.dim() == 1 else int(xs_t.shape[1]))
        if n + G > eng.n_cap:
            raise ValueError(f"choose_inducing_points needs n + G <= n_cap ({n} + {G} > {eng.n_cap})")
        xs_c = xs_t if thin is None else xs_t[thin.to(xs_t.device)]
        xs_s, _ = self._prepare_inputs(xs_c)
        given_s = self._prepare_inputs(g_t)[0] if G else None
        eps = torch.finfo(torch.float32 if eng.pure_fp32 else torch.float64).eps
        floor = max(self._jitter, (G + count) * eps * self._kernel_variance_now(eng))
        out = eng.select_inducing(xs_s, count, given=given_s, floor=floor, return_residual=return_residual)
        idx = out[0]
        idx_all = idx if thin is None else thin.to(idx.device)[idx]
        res = dict(indices=idx_all, points=xs_t.to(idx.device)[idx_all] if xs_t.dim() == 2 else xs_t.to(idx.device)[idx_all].unsqueeze(-1),
                   pivots=out[1], residual_trace=out[2], rank=out[3], floor=floor, scaled=xs_s[idx])
        if return_residual:
            res["residual"] = out[4]
        return res

    def choose_inducing_points(self, xs, count: Optional[int] = None, given=None, max_candidates: int = GREEDY_MAX_CANDIDATES,
                               return_residual: bool = False):
        """Which ``count`` (default: M) rows of ``xs`` to use as inducing points: the greedy conditional-variance selection (Burt, Rasmussen
        and van der Wilk 2020, Alg. 1), the pivoted partial Cholesky of the prior kernel matrix K_nn at the kernel's CURRENT
        hyper-parameters.  Each pick is the row the points chosen so far explain worst, equal values to the lower index.  A dict:
        ``indices`` (count,) int64 into ``xs`` in the order picked; ``points`` (count, D), those rows in the world's coordinates;
        ``pivots`` (G + count,) float64, the conditional prior variance of each pick when it was made (the given rows first), never
        increasing over the free picks; ``residual_trace`` (G + count,) float64, tr(K_nn - Q_nn) after each pick, the quantity the bound
        on the sparse approximation is written in; ``rank``, the picks whose pivot was above the floor max(jitter, (G + count) eps k(x, x))
        (fewer than G + count: the rows hold no more distinct places under this kernel, the later picks explain nothing); ``floor``;
        with ``return_residual`` ``residual`` (n,) float64, diag(K_nn - Q_nn) after the last pick, over the candidate rows.  ``given``
        (G, D), in the world's coordinates like ``xs``: points already there, conditioned on first; with ``count`` = 0 the call scores
        them, e.g. the model's own points (``inducing_points`` is in the scaled world: the same thing for a unit world).  More than
        ``max_candidates`` rows are thinned to the rows floor(i n / max_candidates); ``indices`` still refer to ``xs`` and ``residual`` to
        the thinned rows.  The model is not changed: M is fixed at construction, SparseMultinomialGDRF(inducing_init="greedy") or
        inducing_points=... start a model from such a choice.  All candidates in one call, G + count <= INDUCING_MAX_PICKS."""
        xs_t = torch.as_tensor(xs)
        n_all = int(xs_t.shape[0])
        thin = thin_rows(n_all, max_candidates)
        n = n_all if thin is None else int(thin.numel())
        g_t = None if given is None else torch.as_tensor(given)
        count = self.M if count is None else count
        _, _, G = check_inducing_args(count, None, n, g_t, 1 if xs_t.dim() == 1 else int(xs_t.shape[1]))
        res = self._choose_inducing(self._engine_for(n + G), xs_t, count, g_t, max_candidates, return_residual)
        del res["scaled"]
        return res

    # ------------------------------------------------------------------ fold-in: observed samples from their own counts (csrc/foldin.h)
    def _fold_in(self, xs, ws, mode: int, num_iters, tol, ws_score=None, return_diagnostics: bool = False):
        """Engine.fold_in over row pieces (_mc_pieces; a row's result depends on no other row, so the pieces change nothing but mode 3's
        order of summation); counts that one piece covers go through as the caller's objects.  The pieces are joined along the row axis,
        mode 3's two sums are added; with ``return_diagnostics`` the (3, N) float64 diagnostics - J, |g|_inf / max(1, R), iterations used -
        follow."""
        if self._link_function is not None:
            raise NotImplementedError("fold-in with a custom link_function: the kernel fuses the softmax link")
        n = int(torch.as_tensor(xs).shape[0])
        num_iters, tol = check_fold_args(num_iters, tol, n, self._V, ws, ws_score)
        xs_s, ws_d = self._prepare_inputs(xs, ws)
        sc_d = None if ws_score is None else self._prepare_inputs(xs, ws_score)[1]
        def piece(eng, x, a, b, whole, mean, **draws):          # fold-in draws nothing: the seed, row_offset and eps stay here
            return eng.fold_in(x, count_rows(ws_d, a, b, whole), mode, num_iters, tol, ws_score=count_rows(sc_d, a, b, whole), mean=mean)
        res, diag = self._mc_pieces(xs_s, piece, ({0: 0, 1: 1, 2: 0, 3: None}[mode], 1))
        return (res, diag) if return_diagnostics else res

    def infer_topic_probs(self, xs, ws, num_iters: int = 64, tol: float = 1e-6, return_diagnostics: bool = False):
        """(N, K) topic proportions of the OBSERVED samples (xs, ws): theta_hat = softmax(mu_hat), mu_hat the per-row maximiser of
        sum_v w_v log (softmax(mu) Phi)_v - 1/2 sum_k ((mu_k - m_k) / s_k)^2 reached from mu = m, where m = forward(xs)[0] and
        s = forward(xs)[1] + noise are the location and scale of the model's mu site (LDA's transform with the GP as the prior).
        ``ws``: dense int32 counts or a ``torch.sparse_csr`` matrix.  topic_probs(xs) is softmax(m): it cannot use the counts."""
        return self._fold_in(xs, ws, 0, num_iters, tol, return_diagnostics=return_diagnostics)

    def infer_log_topic_probs(self, xs, ws, num_iters: int = 64, tol: float = 1e-6, return_diagnostics: bool = False):
        """(K, N): mu_hat of infer_topic_probs, laid out as log_topic_probs lays out f_loc."""
        return self._fold_in(xs, ws, 1, num_iters, tol, return_diagnostics=return_diagnostics)

    def topic_counts(self, xs, ws, num_iters: int = 64, tol: float = 1e-6, return_diagnostics: bool = False):
        """(N, K) expected topic counts r_k = theta_k sum_v w_v Phi_kv / p_v at infer_topic_probs' theta_hat: a row sums to its total."""
        return self._fold_in(xs, ws, 2, num_iters, tol, return_diagnostics=return_diagnostics)

    def completion_perplexity(self, x, w_fit, w_score, num_iters: int = 64, tol: float = 1e-6, return_diagnostics: bool = False):
        """The document-completion score exp(-sum w_score log p_hat / sum w_score) as a 0-d tensor: p_hat = theta_hat Phi with theta_hat
        folded in from ``w_fit`` alone; ``w_score`` has the shape and layout (dense or CSR) of ``w_fit``."""
        if w_score is None:
            raise ValueError("completion_perplexity needs w_score, counts of the shape and layout of w_fit")
        res = self._fold_in(x, w_fit, 3, num_iters, tol, ws_score=w_score, return_diagnostics=return_diagnostics)
        s, diag = res if return_diagnostics else (res, None)
        ppl = torch.exp(-s[0] / s[1])
        return (ppl, diag) if return_diagnostics else ppl

    # ------------------------------------------------------------------ joint posterior at new inputs (csrc/predict_cov.h)
    def posterior(self, Xnew) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loc (K, N), cov (K, N, N)) of the GP posterior q(f(Xnew)): what ``gp.util.conditional(..., full_cov=True)`` gives inside
        ``SparseGDRF.forward(Xnew, full_cov=True)`` (gdrf/models/sparse_gdrf.py:277-319), with the mean_function added to loc.  loc is
        ``forward(Xnew)[0]``; the diagonal of cov[k] is ``forward(Xnew)[1][k]`` except that K_** - W W^T is not clamped at 0 here.  Every
        cov[k] equals its transpose to the bit.  All rows at once, at most JOINT_MAX_ROWS of them."""
        check_joint_args(1, self._K, self.M, int(torch.as_tensor(Xnew).shape[0]))
        xs_s, _ = self._prepare_inputs(Xnew)
        eng = self._engine_for(xs_s.shape[0])
        loc = eng.predict(xs_s, 4)[0]
        mean = self._mean_values(xs_s)
        if mean is not None:
            loc = loc + mean.to(loc)
        return loc, eng.predict_cov(xs_s, 0)

    def sample_fields(self, xs, num_samples, seed=None, xi=None, zeta=None) -> torch.Tensor:
        """(S, K, N) joint samples of the latent field f under the GP posterior at the rows ``xs``, mean_function included: every
        sample is one spatially coherent draw over all the rows, f[s, k] ~ N(loc_k, cov_k + j I) with (loc, cov) = posterior(xs) and j the
        jitter the engine had to add to factorise the residual covariance (``_engine.last_joint_jitter``).  ``xi`` (S, K, M) and ``zeta``
        (S, K, N): injected standard normals; otherwise counter-based Philox draws keyed by ``seed`` (default: the model's rng_seed).
        The rows of sample_topic_probs' samples are independent of each other; these are not.  At most JOINT_MAX_ROWS rows."""
        n = int(torch.as_tensor(xs).shape[0])
        S = check_joint_args(num_samples, self._K, self.M, n, xi, zeta)
        xs_s, _ = self._prepare_inputs(xs)
        eng = self._engine_for(n)
        seed = self.rng_seed if seed is None else int(seed)
        inj = [None if t is None else torch.as_tensor(t).to(device=self.device, dtype=self.dtype).contiguous() for t in (xi, zeta)]
        return eng.sample_joint(xs_s, S, seed=seed, xi=inj[0], zeta=inj[1], mean=self._mean_values(xs_s))

    def sample_topic_maps(self, xs, num_samples, seed=None) -> torch.Tensor:
        """(S, N, K) spatially coherent samples of the topic proportions: the link - softmax over the topics, or the custom
        ``link_function`` applied with torch as sample_topic_probs applies it - of the joint field samples ``sample_fields(xs, ...)``.
        The guide's extra noise layer mu ~ Normal(f_loc, f_var), which sample_topic_probs draws per row, is NOT added: a map is the
        link of the latent field itself."""
        check_joint_args(num_samples, self._K, self.M, int(torch.as_tensor(xs).shape[0]))
        f = self.sample_fields(xs, num_samples, seed=seed)
        if self._link_function is not None:
            return torch.stack([self._link_function(f[s]).T for s in range(f.shape[0])])
        return torch.softmax(f, dim=1).transpose(1, 2).contiguous()

    # ------------------------------------------------------------------ posterior-predictive counts (csrc/sample_counts.h)
    def _count_args(self, xs, totals, num_samples, coherent=False, theta=None, u=None, ws=None):
        """The argument errors of sample_counts / predictive_check, raised before the device is touched; returns (S, N, totals as a
        (N,) tensor of integers)."""
        if isinstance(num_samples, bool) or int(num_samples) != num_samples:
            raise ValueError(f"num_samples must be an integer, got {num_samples!r}")
        S, N = int(num_samples), int(torch.as_tensor(xs).shape[0])
        if S < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        if N < 1:
            raise ValueError(f"sample_counts needs at least one row, got {N}")
        if theta is not None and tuple(torch.as_tensor(theta).shape) != (S, N, self._K):
            raise ValueError(f"theta must have shape (num_samples, N, K) = ({S}, {N}, {self._K}), got {tuple(torch.as_tensor(theta).shape)}")
        tot = torch.as_tensor(totals)
        if tot.dim() == 0:
            tot = tot.expand(N)
        check_count_args(torch.empty(S, N, self._K, device="meta"), tot, self._K, self._V, 0 if ws is None else 1, ws,
                         None if u is None else torch.as_tensor(u))
        if coherent and theta is None:
            check_joint_args(S, self._K, self.M, N)
        return S, N, tot

    def _count_theta(self, xs, S: int, seed, coherent: bool, theta) -> torch.Tensor:
        """(S, N, K) topic proportions for the count sampler: injected, one coherent map per sample, or independent rows"""
        if theta is not None:
            return torch.as_tensor(theta).to(device=self.device, dtype=self.dtype).contiguous()
        return self.sample_topic_maps(xs, S, seed=seed) if coherent else self.sample_topic_probs(xs, S, seed=seed)

    def _sample_counts(self, theta: torch.Tensor, totals: torch.Tensor, mode: int, seed, ws_d=None, u=None):
        """Engine.sample_counts over pieces of at most MC_PIECE_ROWS rows, each with its row_offset: the draws are keyed by the global row,
        so the counts do not depend on the piece size.  Mode 0: joined along the row axis; mode 1: the pieces' sums and zero counts added."""
        eng, n = self._engine_for(1), theta.shape[1]
        totals = totals.to(device=self.device, dtype=torch.int32).contiguous()
        if u is not None:
            u = torch.as_tensor(u).to(device=self.device, dtype=torch.float64)
        return join_pieces([eng.sample_counts(theta if whole else theta[:, a:b].contiguous(), totals[a:b], mode, ws=count_rows(ws_d, a, b),
                                              seed=seed, row_offset=a, u=None if u is None else u[:, a:b].contiguous())
                            for a, b, whole in row_pieces(n, MC_PIECE_ROWS)], 1 if mode == 0 else (None, None))

    def sample_counts(self, xs, totals, num_samples, seed=None, coherent=False, theta=None, u=None) -> torch.Tensor:
        """(S, N, V) int32 counts drawn from the fitted model, what ``pyro.infer.Predictive(model, guide=guide, num_samples=S)`` samples at
        the ``w`` site: w_rep[s, n] ~ Multinomial(totals[n], theta[s, n] Phi).  ``totals``: an int or (N,) ints >= 0.  theta comes from
        ``sample_topic_probs(xs, S, seed)`` (independent rows, any N, a custom link_function honoured), with ``coherent=True`` from
        ``sample_topic_maps(xs, S, seed)`` (one spatially coherent field per replicate, at most JOINT_MAX_ROWS rows), or is the injected
        ``theta`` (S, N, K).  ``u``: injected uniforms (S, N, >= max totals) float64 in [0, 1), one per token; otherwise counter-based Philox
        draws keyed by ``seed`` (default: the model's rng_seed) and (row, token, sample), on a stream apart from the one that draws theta."""
        S, _, tot = self._count_args(xs, totals, num_samples, coherent, theta, u)
        seed = self.rng_seed if seed is None else int(seed)
        return self._sample_counts(self._count_theta(xs, S, seed, coherent, theta), tot, 0, seed, u=u)

    def predictive_check(self, xs, ws, num_samples: int = 200, seed=None, coherent=False) -> Dict[str, torch.Tensor]:
        """A posterior predictive check of the dense counts ``ws`` (N, V): ``num_samples`` replicates at the observed row totals, reduced
        on the device without storing them.  With q_s = theta_s Phi of draw s and the deviance D(w; q) = 2 sum_n sum_{v: w > 0} w log(w /
        (T_n q_v)) it returns ``deviance_obs`` (S,) = D(ws; q_s), ``deviance_rep`` (S,) = D(w_rep_s; q_s), ``p_deviance`` = the share of s
        with deviance_rep >= deviance_obs, ``zeros_obs`` (V,) = the rows in which a word is absent, ``zeros_rep`` (S, V) the same for each
        replicate, ``p_zeros`` (V,) = the share of s with zeros_rep >= zeros_obs.  theta and the seed as in sample_counts."""
        check_mc_args(num_samples, self._K, 0, ws=ws)
        wt = torch.as_tensor(ws)
        N = int(torch.as_tensor(xs).shape[0])
        if tuple(wt.shape) != (N, self._V) or wt.dtype.is_floating_point:
            raise ValueError(f"ws must be dense integer counts of shape (N, V) = ({N}, {self._V}), got {wt.dtype} {tuple(wt.shape)}")
        S, _, tot = self._count_args(xs, wt.sum(1), num_samples, coherent, ws=wt)
        seed = self.rng_seed if seed is None else int(seed)
        _, ws_d = self._prepare_inputs(xs, ws)
        dev, zeros_rep = self._sample_counts(self._count_theta(xs, S, seed, coherent, None), tot, 1, seed, ws_d=ws_d)
        zeros_obs = (ws_d == 0).sum(0)
        return dict(deviance_obs=dev[1], deviance_rep=dev[0], p_deviance=(dev[0] >= dev[1]).double().mean(),
                    zeros_obs=zeros_obs, zeros_rep=zeros_rep, p_zeros=(zeros_rep >= zeros_obs[None]).double().mean(0))

    @property
    def word_topic_matrix(self) -> torch.Tensor:
        return torch.softmax(self._engine.view("phi_unc"), dim=-1)

    @property
    def kernel_lengthscale(self):
        if "log_lengthscale" not in self._engine.param_names:
            raise AttributeError("kernel_lengthscale: the model's kernel is a Product; its factors' values are in kernel_parameters")
        return self._engine.view("log_lengthscale").exp().detach().cpu().numpy()

    @property
    def kernel_parameters(self) -> Dict[str, object]:
        """The kernel's constrained parameter values by pyro name, relative to the kernel: {"variance": ..., "lengthscale": ...} for a
        lone kernel, {"kern0.variance": ..., "kern1.period": ...} for a Product.  0-d or 1-d arrays."""
        out = {}
        for n in self._param_names():
            key = state_key(n)
            if key.startswith("_kernel.") and key.endswith("_unconstrained"):
                out[key[len("_kernel."):-len("_unconstrained")]] = self._engine.view(n).exp().detach().cpu().numpy()
        return out

    @property
    def kernel_period(self):
        """The Periodic kernel's period: a 0-d or (D,) array."""
        if self._kernel.name != "periodic":
            raise AttributeError("kernel_period: the model's kernel is not Periodic")
        if "log_period" not in self._engine.param_names:
            raise AttributeError("kernel_period: the model's kernel is a Product; its factors' values are in kernel_parameters")
        return self._engine.view("log_period").exp().detach().cpu().numpy()

    @property
    def kernel_variance(self):
        if "log_variance" not in self._engine.param_names:
            raise AttributeError("kernel_variance: the model's kernel is a Product; its factors' values are in kernel_parameters")
        return self._engine.view("log_variance").exp().detach().cpu().numpy()

    @property
    def noise(self):
        return self._engine.view("log_noise").exp()

    @property
    def u_loc(self):
        return self._engine.view("u_loc")

    @property
    def u_scale_tril(self):
        u = self._engine.view("u_scale_tril_unc")
        return u.tril(-1) + torch.diag_embed(u.diagonal(dim1=-2, dim2=-1).exp())

    def artifacts(self, xs, ws, all: bool = False):
        """gdrf/models/sparse_gdrf.py:146-158: the kernel variance and lengthscale (a (D,) array for an ARD kernel), plus the inducing
        inputs when they are learnable."""
        if isinstance(self._kernel, Product):      # the reference's _get("_kernel.lengthscale") has no such parameter to read
            ret = {f"kernel {k}": v for k, v in self.kernel_parameters.items()}
        else:
            ret = {"kernel variance": self.kernel_variance, "kernel lengthscale": self.kernel_lengthscale}
        if not self._fixed_inducing_points:
            ret["inducing_points"] = self.inducing_points.detach().cpu().numpy()
        return ret

    # ------------------------------------------------------------------ state (train_script.py:338-363,490-506)
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {state_key(n): self._engine.view(n).detach().clone() for n in self._param_names()}

    def _param_names(self):
        return tuple(self._engine.param_names)

    def load_state_dict(self, state: Dict[str, torch.Tensor], strict: bool = True):
        v = {n: self._engine.view(n) for n in self._param_names()}
        if strict:
            unexpected = sorted(k for k in state if k.startswith(MEAN_PREFIX) and k not in v)
            if unexpected:
                raise RuntimeError(f"unexpected keys: {unexpected}")
        missing = []
        for n in self._param_names():
            key = state_key(n)
            if key not in state:
                missing.append(key)
                continue
            t = torch.as_tensor(state[key])
            if tuple(t.shape) != tuple(v[n].shape):
                if strict:
                    raise RuntimeError(f"size mismatch for {key}: {tuple(t.shape)} vs {tuple(v[n].shape)}")
                continue
            v[n].copy_(t.to(v[n]))
        if strict and missing:
            raise RuntimeError(f"missing keys: {missing}")
        self._mean_to_module()
        return missing

    def parameters(self):
        return [self._engine.view(n) for n in self._param_names()]

    def float(self):
        return self

    def __deepcopy__(self, memo):
        """``deepcopy(model)`` (train_script.py:493): a ModelSnapshot - parameters plus what a loaded checkpoint needs to rebuild
        the predictive surface (gdrf/utils/loggers.py:35-47)."""
        self._engine.refresh_inducing()
        meta = dict(K=self._K, V=self._V, M=self.M, D=self.D, world=[list(w) for w in self._world], kernel=self._kernel.name,
                    n_points=list(self._n_points), fixed_inducing_points=self._fixed_inducing_points, whiten=self._whiten,
                    jitter=self._jitter, maxjitter=self._maxjitter, dirichlet_param=self._dirichlet_param.detach().cpu().clone(),
                    inducing_points=self._engine.Z.detach().cpu().clone(), dtype=str(self.dtype).replace("torch.", ""),
                    device=str(self.device), pure_fp32=self._pure_fp32, mfma_mode=self._mfma_mode, seed=self.rng_seed,
                    guide_rescale=self._guide_rescale, rows_form=self._rows_form,
                    kernel_spec=kernel_spec(self._kernel))
        return ModelSnapshot(self.state_dict(), meta)


# The model methods a ModelSnapshot offers by forwarding to the device model it rebuilds; a new predictive method joins by its name.
SNAPSHOT_METHODS = (
    "log_topic_probs", "topic_probs", "word_probs", "perplexity", "sample_topic_probs", "topic_probs_mc", "word_probs_mc",
    "predictive_perplexity", "pointwise_log_likelihood", "waic", "row_perplexity", "information", "most_informative",
    "topic_probs_quantiles", "word_probs_quantiles", "exceedance", "dominant_topic_probs", "select_batch", "infer_topic_probs",
    "infer_log_topic_probs", "topic_counts", "completion_perplexity", "posterior", "sample_fields", "sample_topic_maps", "sample_counts",
    "predictive_check")


def _snapshot_method(name: str):
    """``ModelSnapshot.name``: the model's method on ``restore()``, under the model method's signature and docstring"""
    @functools.wraps(getattr(SparseMultinomialGDRF, name))
    def method(self, *args, **kwargs):
        return getattr(self.restore(), name)(*args, **kwargs)
    method.__qualname__ = f"ModelSnapshot.{name}"
    return method


# Forwarded the same way, but no predictive method: it reads the kernel's hyper-parameters alone and chooses points for ANOTHER model
SNAPSHOT_SETUP_METHODS = ("choose_inducing_points",)

for _name in SNAPSHOT_METHODS + SNAPSHOT_SETUP_METHODS:
    setattr(ModelSnapshot, _name, _snapshot_method(_name))
