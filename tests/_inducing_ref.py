"""A float64 numpy restatement of the greedy conditional-variance choice of inducing points (gdrf_select_inducing,
csrc/select_inducing.h), in two independent forms:

* ``greedy``: the loop of the definition.  d[j] = k(x_j, x_j); pick t is the t-th given row, else the candidate not picked yet with the
  largest d (ties to the lower index), or the row ``forced`` names - which conditions the loop on somebody else's picks -;
  piv = d[p]; above the floor c_t = (k(., x_p) - sum_s c_s c_s[p]) / sqrt(piv) and d -= c_t^2, else c_t = 0; trace_t = sum_{j<n} d[j].
* ``nystrom_residual``: diag(K_nn - K_nP K_PP^-1 K_Pn) by a dense solve, for any list of points P.  It knows nothing of the loop.

``Kern`` is a kernel of every kind a context supports at hyper-parameters whose logarithms the context's element type holds exactly: the
same numbers go to the engine (``Kern.log``, by the names of Engine.view) and into the float64 formulas here (pyro's isotropic kernels with
the 1e-12 under the root, ARD as scaled coordinates, Periodic and Product as the RBF kernel on the embedded coordinates).  No device."""
import math

import numpy as np

ISOTROPIC = ("rbf", "matern52", "matern32", "exponential", "rationalquadratic")
KINDS = ISOTROPIC + ("ard", "periodic", "product")
VAR = 25.0


def iso_cov(kind, r2, var, alpha=1.0):
    if kind == "rbf":
        return var * np.exp(-0.5 * r2)
    if kind == "rationalquadratic":
        return var * (1.0 + r2 * (0.5 / alpha)) ** (-alpha)
    r = np.sqrt(r2 + 1e-12)
    if kind == "exponential":
        return var * np.exp(-r)
    if kind == "matern32":
        return var * (1.0 + math.sqrt(3.0) * r) * np.exp(-math.sqrt(3.0) * r)
    if kind == "matern52":
        return var * (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * r * r) * np.exp(-math.sqrt(5.0) * r)
    raise ValueError(kind)


class Kern:
    """kind: one of KINDS.  "ard": RBF with one lengthscale per axis; "periodic": D <= 2, one period; "product": RBF on axis 0 times Periodic
    on axis 1 (D = 2).  dtype: "float64" or "float32", the element type of the context whose parameters these are."""

    def __init__(self, kind, D=2, dtype="float64", ls=0.3, var=VAR, alpha=1.5, period=0.45):
        assert kind in KINDS
        self.kind, self.D, self.dtype = kind, D, dtype
        lg = lambda v: np.log(np.asarray(v, dtype=np.float64)).astype(dtype).astype(np.float64)
        if kind in ISOTROPIC:
            self.log = dict(log_lengthscale=lg(ls), log_variance=lg(var))
            if kind == "rationalquadratic":
                self.log["log_scale_mixture"] = lg(alpha)
        elif kind == "ard":
            self.log = dict(log_lengthscale=lg([ls * (1 + 0.25 * d) for d in range(D)]), log_variance=lg(var))
        elif kind == "periodic":
            assert D <= 2
            self.log = dict(log_lengthscale=lg(0.8), log_variance=lg(var), log_period=lg(period))
        else:
            assert D == 2
            self.log = {"kern0.log_variance": lg(5.0), "kern0.log_lengthscale": lg(ls), "kern1.log_variance": lg(var / 5.0),
                        "kern1.log_lengthscale": lg(0.8), "kern1.log_period": lg(period)}
        self.val = {k: np.exp(v) for k, v in self.log.items()}

    @property
    def variance(self):
        """k(x, x) but for the 1e-12 under the root: what bounds and floors are relative to"""
        return float(np.prod([v for k, v in self.val.items() if k.endswith("log_variance")]))

    def engine_kwargs(self):
        """(kernel name, keyword arguments) of gdrf_amd.engine.Engine"""
        if self.kind == "ard":
            return "rbf", dict(ard=True)
        if self.kind == "periodic":
            return "periodic", dict(period_count=1)
        if self.kind == "product":
            return "product", dict(product=[dict(name="kern0", kind="rbf", active_dims=[0], lengthscales=1, periods=0),
                                            dict(name="kern1", kind="periodic", active_dims=[1], lengthscales=1, periods=1)])
        return self.kind, {}

    def coords(self, X):
        """(base kind, coordinates e(x)): k(x, y) = iso_cov(base kind, |e(x) - e(y)|^2, variance)"""
        X, v = np.asarray(X, dtype=np.float64), self.val
        if self.kind in ISOTROPIC or self.kind == "ard":
            return ("rbf" if self.kind == "ard" else self.kind), X / v["log_lengthscale"]
        if self.kind == "periodic":
            t = 2 * math.pi / v["log_period"]
            return "rbf", np.concatenate([np.cos(t * X), np.sin(t * X)], 1) / v["log_lengthscale"]
        t = 2 * math.pi / v["kern1.log_period"]
        return "rbf", np.concatenate([X[:, :1] / v["kern0.log_lengthscale"], np.cos(t * X[:, 1:]) / v["kern1.log_lengthscale"],
                                      np.sin(t * X[:, 1:]) / v["kern1.log_lengthscale"]], 1)

    def __call__(self, X, Y):
        kind, ex = self.coords(X)
        _, ey = self.coords(Y)
        r2 = np.zeros((ex.shape[0], ey.shape[0]))
        for d in range(ex.shape[1]):                     # the direct (x - y)^2 form, an axis at a time: no (n, n, D) array
            r2 += (ex[:, d:d + 1] - ey[None, :, d]) ** 2
        return iso_cov(kind, r2, self.variance, float(self.val.get("log_scale_mixture", 1.0)))

    def diag(self):
        z = np.zeros((1, self.D))
        return float(self(z, z)[0, 0])


def greedy(kern, X, count, given=None, floor=0.0, forced=None):
    """The loop of the definition on the rows X (n, D) with the G given rows appended as forced pivots.  ``forced``: the rows to take as the
    free picks instead of the loop's own argmax (the loop is then conditioned on them; ``best`` still says what it would have taken).
    Returns a dict: picks (count), pivots, trace (G + count each), rank, d (n) after the last pick, best (count): the largest d among the
    candidates not picked yet at each free pick, gap: the smallest lead of that d over the runner-up (inf with one candidate; the very
    first pick of a run without given rows does not count: all d are then one and the same number, on the device too, and row 0 is taken)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    G = 0 if given is None else int(np.asarray(given).shape[0])
    Xa = X if not G else np.concatenate([X, np.asarray(given, dtype=np.float64).reshape(G, X.shape[1])])
    nt, T = n + G, G + count
    d = np.full(nt, kern.diag())
    c = np.zeros((T, nt))
    free = np.ones(n, dtype=bool)
    picks, pivots, trace, best, rank, gap = [], [], [], [], 0, float("inf")
    for t in range(T):
        if t < G:
            p = n + t
        else:
            cand = np.where(free, d[:n], -np.inf)
            order = np.argmax(cand)                      # the first of equal values: ties to the lower index
            top = float(cand[order])
            if free.sum() > 1 and t > 0:                 # pick 0 without given rows: every d is the same number, the tie goes to row 0
                rest = cand.copy()
                rest[order] = -np.inf
                gap = min(gap, top - float(rest.max()))
            best.append(top)
            p = int(order) if forced is None else int(forced[t - G])
            assert free[p], (t, p)
            free[p] = False
            picks.append(p)
        piv = float(d[p])
        pivots.append(piv)
        if piv > floor:
            col = kern(Xa, Xa[p:p + 1])[:, 0]
            c[t] = (col - c[:t].T @ c[:t, p]) / math.sqrt(piv)
            d = d - c[t] ** 2
            rank += 1
        trace.append(float(d[:n].sum()))
    return dict(picks=picks, pivots=np.array(pivots), trace=np.array(trace), rank=rank, d=d[:n].copy(), best=np.array(best), gap=gap)


def nystrom_residual(kern, X, P):
    """diag(K_nn - K_nP K_PP^-1 K_Pn) (n,) for the points P (m, D), by a dense solve"""
    X, P = np.asarray(X, dtype=np.float64), np.asarray(P, dtype=np.float64)
    if P.shape[0] == 0:
        return np.full(X.shape[0], kern.diag())
    KnP = kern(X, P)
    return kern.diag() - (KnP * np.linalg.solve(kern(P, P), KnP.T).T).sum(1)


def uniform_rows(seed, n, D):
    return np.random.default_rng(seed).random((n, D))


# The float64 cases in which the device must make the restatement's own picks: (seed, n, D, M, kind, lengthscale); at every step the best d
# leads the runner-up by at least EXACT_GAP of the variance (asserted on the CPU, tests/test_select_inducing_host.py)
EXACT_CASES = [(0, 300, 2, 64, "rbf", 0.2), (1, 257, 1, 33, "matern52", 0.3), (2, 513, 3, 96, "rbf", 0.3), (3, 300, 2, 64, "exponential", 0.2)]
EXACT_GAP = 1e-9


def spiral_track():
    """600 rows on a noisy spiral track in the unit square"""
    rng = np.random.default_rng(7)
    t = np.sort(rng.random(600))
    X = np.stack([0.5 + 0.45 * t * np.cos(6 * np.pi * t), 0.5 + 0.45 * t * np.sin(6 * np.pi * t)], 1) + 0.005 * rng.standard_normal((600, 2))
    return np.clip(X, 0.0, 1.0)


def mesh(m, D=2):
    """the m^D tensor-product mesh over [0, 1]^D, last axis fastest"""
    ax = np.linspace(0.0, 1.0, m)
    return np.stack([a.ravel() for a in np.meshgrid(*([ax] * D), indexing="ij")], 1)


def duplicated_rows(seed=11, places=40, copies=3, D=2):
    """``places`` distinct rows, each present ``copies`` times: the whole set, then again, then again (row i's twins are i + places, ...)"""
    a = uniform_rows(seed, places, D)
    return np.concatenate([a] * copies)
