"""A float64 torch restatement of the batch choice (gdrf_select_batch, csrc/select_batch.h), written from its DEFINITION and not from the
kernel's recursion.  With C_k = R + T_k T_k^T the joint posterior covariances (R = K_** - W W^T, T_k = W S_k; whiten=False: L^-1 S_k) and s2
the observation-noise variance, the variance of f_k(x_j) given noisy observations at the rows A is

    d_k[j] = C_k[j][j] - C_k[j, A] (C_k[A, A] + s2 I)^-1 C_k[A, j]

by a dense solve at every step; the gain of row j is 1/2 sum_k log1p(max(d_k[j], 0) / s2) and the greedy rule picks the largest gain among
the rows not picked yet, ties to the lower index.  A is the given rows followed by the picks so far.  Only the columns C_k[:, A] and the
diagonal are formed - no n x n matrix -, so the restatement also serves n = 2^16 + 1.

``case`` is a ``tests.test_gpu_joint.Case`` (or the Case-shaped object of its ``model_case``): it supplies the kernel function on float64
values that the context's element type holds exactly, Z, u, S and the engine whose K_uu jitter level is used."""
import torch

from oracle.gdrf_oracle import jittercholesky


class SelectRef:
    def __init__(self, case, X, s2, given=None):
        X = torch.as_tensor(X, dtype=torch.float64)
        self.n = X.shape[0]
        self.G = 0 if given is None else int(given.shape[0])
        self.X = X if not self.G else torch.cat([X, torch.as_tensor(given, dtype=torch.float64)])
        self.s2, self.case = float(s2), case
        eng = case.eng
        L, _ = jittercholesky(case.kfun(case.Z, case.Z), case.M, eng.jitter, eng.maxjitter, force_level=eng.last_jitter_level)
        self.W = torch.linalg.solve_triangular(L, case.kfun(case.Z, self.X), upper=False).T          # (nt, M)
        S = case.S if case.whiten else torch.linalg.solve_triangular(L[None], case.S, upper=False)
        self.T = self.W[None] @ S                                                                     # (K, nt, M)
        kdiag = case.kfun(self.X[:1], self.X[:1])[0, 0]                                               # a stationary kernel: k(x, x) is one number
        self.diag = (kdiag - (self.W ** 2).sum(1))[None] + (self.T ** 2).sum(2)                       # (K, nt): diag C_k
        self.given = list(range(self.n, self.n + self.G))

    def columns(self, A):
        """C_k[:, A] as (K, nt, |A|)"""
        RA = self.case.kfun(self.X, self.X[A]) - self.W @ self.W[A].T
        return RA[None] + self.T @ self.T[:, A].transpose(1, 2)

    def cond_var(self, picks):
        """d (K, nt) given noisy observations at the given rows and ``picks``"""
        A = self.given + [int(p) for p in picks]
        if not A:
            return self.diag.clone()
        CA = self.columns(A)
        CAA = CA[:, A, :] + self.s2 * torch.eye(len(A), dtype=torch.float64)
        sol = torch.linalg.solve(CAA, CA.transpose(1, 2))                                             # (K, |A|, nt)
        return self.diag - (CA * sol.transpose(1, 2)).sum(2)

    def gains(self, picks):
        """(n,) gains of the candidates given ``picks`` (-inf for a picked row)"""
        d = self.cond_var(picks)[:, :self.n]
        g = 0.5 * torch.log1p(d.clamp_min(0.0) / self.s2).sum(0)
        if len(picks):
            g[torch.as_tensor([int(p) for p in picks])] = -float("inf")
        return g

    def greedy(self, count):
        """(picks, gains, the smallest relative gap between the best and the second-best gain over the steps)"""
        picks, gains, gap = [], [], float("inf")
        for _ in range(count):
            g = self.gains(picks)
            top = torch.topk(g, min(2, self.n))
            best = float(top.values[0])
            p = int((g == best).nonzero()[0, 0])                                                      # ties to the lower index
            if top.values.numel() > 1 and bool(torch.isfinite(top.values[1])):
                gap = min(gap, (best - float(top.values[1])) / best if best > 0 else 0.0)
            picks.append(p)
            gains.append(best)
        return picks, torch.tensor(gains, dtype=torch.float64), gap

    def information(self, picks):
        """I(given + picks) - I(given): what the free picks' gains add up to"""
        def info(A):
            if not A:
                return 0.0
            CAA = self.columns(A)[:, A, :]
            return float(0.5 * torch.logdet(torch.eye(len(A), dtype=torch.float64)[None] + CAA / self.s2).sum())
        return info(self.given + [int(p) for p in picks]) - info(self.given)
