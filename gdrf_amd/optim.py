"""``pyro.optim`` optimizers as built at gdrf/train_script.py:73-87,325-327: ``OPTIMIZER_DICT[name](optim_args, clip_args)``.

Pyro keeps one torch optimizer per unconstrained parameter tensor, all stepping together.  The HIP path applies the update to the
flat parameter vector: plain Adam / AdamW / ClippedAdam (no ``clip_args``, ``optim_args`` a dict) in one launch of gdrf_adam
(arithmetic in SURVEY.md A.5); every other case through gdrf_optim_step, which takes one table entry per parameter tensor (its
segment of the vector and the step's scalars, computed here in double) and so applies pyro's per-parameter ``optim_args``
callables and ``clip_args`` (DESIGN.md "Optimizers").  ``get_state``/``set_state`` (train_script.py:348,495) expose per-parameter
``{"step", <torch's state keys>, "lr"}``.
"""
from __future__ import annotations

from typing import Dict

import torch

from .engine import OPT_CENTERED, OPT_CLIP_NORM, OPT_CLIP_VALUE, OPT_MODES, OPT_MOMENTUM

CLIP_KEYS = ("clip_norm", "clip_value")


def param_store_name(name: str) -> str:
    """The name pyro's param store gives an engine parameter, as an ``optim_args`` / ``clip_args`` callable receives it: the
    state-dict name without its ``_unconstrained`` suffix ("u_loc", "_kernel.lengthscale", "_mean_function.w")."""
    from .models.sparse_gdrf import state_key
    key = state_key(name)
    return key[:-len("_unconstrained")] if key.endswith("_unconstrained") else key


class PyroOptimLike:
    mode = "adam"                  # update rule (engine.OPT_RULES)
    defaults: Dict[str, object] = {}
    lr_key = "lr"                  # the argument get_state reports as "lr"

    def __init__(self, optim_args=None, clip_args=None):
        # pyro.optim.PyroOptim: a callable is asked once per parameter, fn(module_name, param_name); its dict replaces the arguments
        self._args_fn = optim_args if callable(optim_args) else None
        self.args = dict(self.defaults) if self._args_fn else self._check_args(optim_args or {})
        self._clip_fn = clip_args if callable(clip_args) else None
        self.clip_args = {} if self._clip_fn else self._check_clip(clip_args or {})
        self.lr = float(self.args[self.lr_key])
        self._engine = None
        self._pending_state = None
        self._seg_args: Dict[str, dict] = {}
        self._seg_clip: Dict[str, dict] = {}
        self._host: Dict[str, dict] = {}        # per parameter: the host scalars of its optimizer ("lr"; ASGD's "eta", "mu")

    @classmethod
    def _check_args(cls, given) -> dict:
        if not isinstance(given, dict):
            raise TypeError(f"optimizer arguments must be a dict, got {type(given).__name__}")
        unknown = set(given) - set(cls.defaults)
        if unknown:
            raise ValueError(f"unsupported optimizer arguments: {sorted(unknown)}")
        args = dict(cls.defaults)
        args.update(given)
        return args

    @staticmethod
    def _check_clip(given) -> dict:
        if not isinstance(given, dict):
            raise TypeError(f"clip_args must be a dict, got {type(given).__name__}")
        unknown = set(given) - set(CLIP_KEYS)
        if unknown:
            raise ValueError(f"unsupported clip_args: {sorted(unknown)}; pyro accepts clip_norm and clip_value")
        out = {}
        for k, v in given.items():
            if v is None:
                continue
            v = float(v)
            if not v >= 0.0:
                raise ValueError(f"{k} must be >= 0, got {v}")
            out[k] = v
        return out

    @property
    def segmented(self) -> bool:
        """True when the update goes through gdrf_optim_step (per-parameter scalars), False for the single gdrf_adam launch."""
        return not (self.mode in OPT_MODES and self._args_fn is None and self._clip_fn is None and not self.clip_args)

    def args_for(self, name: str) -> dict:
        """The optimizer arguments of the engine parameter ``name`` (a callable ``optim_args`` is asked once per parameter)."""
        if self._args_fn is None:
            return self.args
        if name not in self._seg_args:
            pn = param_store_name(name)
            self._seg_args[name] = self._check_args(self._args_fn(pn, pn))
        return self._seg_args[name]

    def clip_for(self, name: str) -> dict:
        """The ``clip_args`` of the engine parameter ``name`` ({} = no clipping)."""
        if self._clip_fn is None:
            return self.clip_args
        if name not in self._seg_clip:
            pn = param_store_name(name)
            self._seg_clip[name] = self._check_clip(self._clip_fn(pn, pn) or {})
        return self._seg_clip[name]

    def _host_for(self, name: str) -> dict:
        h = self._host.get(name)
        if h is None:
            lr = float(self.args_for(name)[self.lr_key])
            h = self._host[name] = {"lr": lr, "eta": lr, "mu": 1.0}
        return h

    # -- rule tables: which state vector holds each of torch's state keys (1 exp_avg, 2 exp_avg_sq, 3 opt_extra), its initial value,
    #    the step's scalars and flags (include/gdrf_hip.h, gdrf_optim_step), and what the host updates after the step
    def _slots(self, args: dict) -> Dict[str, int]:
        return {"exp_avg": 1, "exp_avg_sq": 2}

    def _initial(self, args: dict, host: dict, key: str) -> float:
        return 0.0

    def _scalars(self, args: dict, host: dict, t: int):
        b1, b2 = args["betas"]
        clip = float(args.get("clip_norm", 10.0))
        return [host["lr"], b1, b2, args["eps"], float(args.get("weight_decay", 0.0)), clip, 1.0 - b1 ** t, 1.0 - b2 ** t], 0

    def _advance(self, args: dict, host: dict, t: int):
        pass

    # -- bound by SVI at its first step
    def _bind(self, engine):
        if self._engine is engine:
            return
        self._engine = engine
        if self._pending_state is not None:
            self.set_state(self._pending_state)
            self._pending_state = None

    def _step(self):
        e = self._engine
        if not self.segmented:
            a = self.args
            if self.mode == "clippedadam":
                self.lr *= float(a["lrd"])         # pyro's ClippedAdam decays lr BEFORE it forms step_size
            e.adam(self.mode, self.lr, betas=tuple(a["betas"]), eps=float(a["eps"]),
                   weight_decay=float(a.get("weight_decay", 0.0)), clip=float(a.get("clip_norm", 10.0)))
            return
        if e.opt_step == 0:
            self._init_state(e)
        t = e.opt_step + 1
        segs, done = [], []
        for name, (off, n) in e.segments().items():
            args, clip, host = self.args_for(name), self.clip_for(name), self._host_for(name)
            a, flags = self._scalars(args, host, t)
            if "clip_norm" in clip:
                flags |= OPT_CLIP_NORM
            if "clip_value" in clip:
                flags |= OPT_CLIP_VALUE
            if 3 in self._slots(args).values():
                e.state_buffer(3)
            segs.append(dict(offset=off, length=n, a=a, flags=flags, clip_norm=clip.get("clip_norm", 0.0),
                             clip_value=clip.get("clip_value", 0.0)))
            done.append((args, host))
        e.optim_step(self.mode, segs)
        for args, host in done:
            self._advance(args, host, t)

    def _init_state(self, e):
        """torch's state at the first step: every state tensor at its initial value, the host scalars from the arguments."""
        self._host.clear()
        for name in e.param_names:
            args, host = self.args_for(name), self._host_for(name)
            for key, slot in self._slots(args).items():
                e.view(name, e.state_buffer(slot)).fill_(self._initial(args, host, key))

    def get_state(self) -> dict:
        e = self._engine
        if e is None:
            return self._pending_state or {}
        out = {}
        for name in e.param_names:
            args = self.args_for(name)
            st = {"step": e.opt_step}
            for key, slot in self._slots(args).items():
                st[key] = e.view(name, e.state_buffer(slot)).detach().clone()
            if self.segmented:
                host = self._host_for(name)
                if self.mode == "asgd":
                    st["eta"], st["mu"] = host["eta"], host["mu"]
                st["lr"] = host["lr"]
            else:
                st["lr"] = self.lr
            out[name] = st
        return out

    def set_state(self, state: dict):
        e = self._engine
        if e is None:
            self._pending_state = state
            return
        names = set(e.param_names)
        for name, st in state.items():
            if name not in names:
                continue
            args = self.args_for(name)
            for key, slot in self._slots(args).items():
                if key in st:
                    v = e.view(name, e.state_buffer(slot))
                    v.copy_(torch.as_tensor(st[key]).to(v))
            e.opt_step = int(st["step"])
            if self.segmented:
                host = self._host_for(name)
                host["lr"] = float(st.get("lr", host["lr"]))
                for k in ("eta", "mu"):
                    if k in st:
                        host[k] = float(st[k])
            self.lr = float(st.get("lr", self.lr))


class Adam(PyroOptimLike):
    mode = "adam"
    defaults = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


class AdamW(PyroOptimLike):
    mode = "adamw"
    defaults = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


class ClippedAdam(PyroOptimLike):
    mode = "clippedadam"
    defaults = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, clip_norm=10.0, lrd=1.0)

    def _scalars(self, args, host, t):
        host["lr"] *= float(args["lrd"])           # decayed BEFORE it forms the step, as on the gdrf_adam path
        return super()._scalars(args, host, t)


class Adamax(PyroOptimLike):
    """torch.optim.Adamax: u = max(beta2 u, |g| + eps), p -= lr / (1 - beta1^t) m / u."""
    mode = "adamax"
    defaults = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)

    def _slots(self, args):
        return {"exp_avg": 1, "exp_inf": 2}

    def _scalars(self, args, host, t):
        b1, b2 = args["betas"]
        return [host["lr"] / (1.0 - b1 ** t), b1, b2, args["eps"], args["weight_decay"]], 0


class RMSprop(PyroOptimLike):
    """torch.optim.RMSprop, centered and with momentum."""
    mode = "rmsprop"
    defaults = dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False)

    def _slots(self, args):
        s = {"square_avg": 2}
        if args["momentum"] > 0:
            s["momentum_buffer"] = 1
        if args["centered"]:
            s["grad_avg"] = 3 if args["momentum"] > 0 else 1
        return s

    def _scalars(self, args, host, t):
        flags = (OPT_MOMENTUM if args["momentum"] > 0 else 0) | (OPT_CENTERED if args["centered"] else 0)
        return [host["lr"], args["alpha"], args["eps"], args["weight_decay"], args["momentum"]], flags


class Adagrad(PyroOptimLike):
    """torch.optim.Adagrad: sum += g^2, p -= lr / (1 + (t - 1) lr_decay) g / (sqrt(sum) + eps)."""
    mode = "adagrad"
    defaults = dict(lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10)

    def _slots(self, args):
        return {"sum": 2}

    def _initial(self, args, host, key):
        return float(args["initial_accumulator_value"])

    def _scalars(self, args, host, t):
        return [host["lr"] / (1.0 + (t - 1) * args["lr_decay"]), args["eps"], args["weight_decay"]], 0


class Adadelta(PyroOptimLike):
    mode = "adadelta"
    defaults = dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0)

    def _slots(self, args):
        return {"square_avg": 2, "acc_delta": 1}

    def _scalars(self, args, host, t):
        return [host["lr"], args["rho"], args["eps"], args["weight_decay"]], 0


class ASGD(PyroOptimLike):
    """torch.optim.ASGD: the step uses the stored eta and mu; afterwards eta = lr / (1 + lambd lr t)^alpha, mu = 1 / max(1, t - t0)."""
    mode = "asgd"
    defaults = dict(lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0.0)

    def _slots(self, args):
        return {"ax": 1}

    def _scalars(self, args, host, t):
        return [host["eta"], host["mu"], args["lambd"], args["weight_decay"]], 0

    def _advance(self, args, host, t):
        host["eta"] = host["lr"] / ((1.0 + args["lambd"] * host["lr"] * t) ** args["alpha"])
        host["mu"] = 1.0 / max(1.0, t - args["t0"])


class Rprop(PyroOptimLike):
    mode = "rprop"
    defaults = dict(lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50.0))

    def _slots(self, args):
        return {"prev": 1, "step_size": 2}

    def _initial(self, args, host, key):
        return host["lr"] if key == "step_size" else 0.0

    def _scalars(self, args, host, t):
        (em, ep), (smin, smax) = args["etas"], args["step_sizes"]
        return [em, ep, smin, smax], 0


class AdagradRMSProp(PyroOptimLike):
    """pyro.optim.AdagradRMSProp (pyro 1.8.0): sum = g^2 at the first step, then (1 - t) sum + t g^2;
    p -= eta step^(-1/2 + delta) g / (1 + sqrt(sum)).  It has no ``lr`` argument."""
    mode = "adagradrmsprop"
    defaults = dict(eta=1.0, delta=1e-16, t=0.1)
    lr_key = "eta"

    def _slots(self, args):
        return {"sum": 2}

    def _scalars(self, args, host, t):
        return [host["lr"] * t ** (-0.5 + args["delta"]), args["t"], 1.0 if t == 1 else 0.0], 0


def _unsupported(name):
    class _U:
        def __init__(self, *a, **k):
            raise NotImplementedError(f"pyro.optim.{name} is a registry entry of the reference (train_script.py:73-87) that this build "
                                      "does not run; supported: " + ", ".join(sorted(_SUPPORTED)))
    _U.__name__ = name
    return _U


_SUPPORTED = {"adam": Adam, "adamw": AdamW, "clippedadam": ClippedAdam, "adamax": Adamax, "rmsprop": RMSprop, "adagrad": Adagrad,
              "adadelta": Adadelta, "asgd": ASGD, "rprop": Rprop, "adagradrmsprop": AdagradRMSProp}
OPTIMIZER_DICT = dict(_SUPPORTED)
for _n in ["DCTAdam", "SparseAdam", "SGD"]:
    OPTIMIZER_DICT[_n.lower()] = _unsupported(_n)
