"""GPU tests of the per-row ELBO kernels (rows_mfma.h: elbo_rows_mfma_kernel; rows_lds.h: elbo_rows_kernel) at the edges of
their dispatch and of their tiles, against the fp64 reference at the same parameters and the same jitter level.

The host picks the form from (K, V): the matrix-core form <NKT, NVT> for K <= 16 / <= 32 and V <= 32 / <= 64, the one-thread-per-row
kernel with register topics for K <= 32 and larger V, and its LDS-topic form for K > 32.  The matrix-core form works on tiles of 16
topics x 16 words x 16 rows and re-reads clamped topics (K - 1), words (V - 1) and rows (the last one) in the padding lanes; the test
data puts the largest values exactly there, so that a duplicate that leaked into a sum would be far outside the tolerances.
"""
import gc

import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import _np_kernel, fused_elbo_and_grads, jitter_total
from tests._util import dev, engine_from_oracle, make_oracle, relerr
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

JITTER = {torch.float64: 1e-6, torch.float32: 1e-4}


def _aux(m, eps, level, n_global=None, dup_last=False):
    """fp64 reference of one step at the oracle's parameters; dup_last counts the last row twice (with n_global = N unchanged)."""
    P = {k: v.detach().double().numpy().copy() for k, v in m.params.items()}
    xs, ws, e = m.xs.double().numpy(), m.ws.numpy(), eps.double().numpy()
    if dup_last:
        xs, ws, e = np.concatenate([xs, xs[-1:]]), np.concatenate([ws, ws[-1:]]), np.concatenate([e, e[:, -1:]], 1)
    return fused_elbo_and_grads(m.kind, xs, ws, m.Z.double().numpy(), P, m.alpha.double().numpy(), e,
                                jitter_total(m.jitter, level), n_global=n_global)


def _loud_oracle(K, V, W, H, dtype, seed=3):
    """Oracle on a W x H lattice whose data make every clamped duplicate of the matrix-core form visible:
    the last row (re-read by the ragged row group) has ~100x the counts of the others, word V-1 (the clamped word) the largest
    counts of every row, topic K-1 (the clamped topic) dominates the softmax, and a few rows have no counts at all (w == 0)."""
    # a contracted guide (trained_scale) and a wide lengthscale keep v = var - q + tt small, so that eps does not decide the softmax
    m, eps = make_oracle(W=W, H=H, V=V, K=K, n_points=(4, 3), dtype=dtype, seed=seed, jitter=JITTER[dtype], lengthscale=0.3,
                         trained_scale=0.1)
    N = m.N
    rng = np.random.default_rng(seed)
    ws = rng.integers(0, 8, size=(N, V))
    ws[:, V - 1] += rng.integers(20, 60, size=N)
    ws[N - 1] *= 100
    ws[rng.choice(N - 1, size=3, replace=False)] = 0
    m.ws = torch.from_numpy(ws.astype(np.int32))
    # whitened guide: f_k = W u_k with W L^T = K_nm, so u_{K-1} += L^T c lifts f_{K-1} by K_nm c > 0 everywhere: topic K-1 is the
    # largest on ~85 % of the rows, without saturating the softmax
    ls, var = float(m.params["log_lengthscale"].detach().exp()), float(m.params["log_variance"].detach().exp())
    Z = m.Z.double().numpy()
    L = np.linalg.cholesky(_np_kernel(m.kind, Z, Z, ls, var)[0] + m.jitter * np.eye(m.M))
    with torch.no_grad():
        m.params["u_loc"][K - 1] += torch.from_numpy(L.T @ np.full(m.M, 0.2)).to(dtype)
    return m, eps


def _step(eng, m, eps):
    xs, ws, e = dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng)
    eng.loss_and_grads(xs, ws, e)
    out = eng.read_out()
    assert out["chol_failed"] == 0
    n = m.N
    rows = {name: eng.workspace(name, n).cpu().double().numpy() for name in ("q", "mu", "vbar", "locbar")}
    grads = {name: v.cpu().double().numpy() for name, v in eng.named_views(eng.grads).items()}
    return out["loss"], rows, grads


def _assert_close(loss, rows, grads, loss_ref, rows_ref, g_ref, t):
    """loss, the row-kernel outputs and every gradient block, held to the parity table (vbar / locbar at 10 w)"""
    report = {name: relerr(rows[name], rows_ref[name]) for name in rows}
    for name in grads:
        report["g_" + name] = relerr(grads[name], g_ref[name])
    report["loss"] = abs(loss - loss_ref) / abs(loss_ref)
    print({k: f"{v:.2e}" for k, v in report.items()})
    for name in ("q", "mu"):
        assert report[name] < t["w"], (name, report)
    for name in ("vbar", "locbar"):
        assert report[name] < t["w"] * 10, (name, report)
    for name in grads:
        assert report["g_" + name] < t["g"], (name, report)
    assert report["loss"] < t["loss"], report
    return report


def _check_vs_reference(m, eps, level, loss, rows, grads, t):
    """against the fp64 reference at the oracle's parameters and the engine's jitter level; returns the reference (loss, grads, aux)"""
    loss_ref, g_ref, aux = _aux(m, eps, level)
    _assert_close(loss, rows, grads, loss_ref, aux, g_ref, t)
    return loss_ref, g_ref, aux


# two (K, V) pairs per form, at the edges of its range; comment: the form the host picks
SWEEP = [
    (1, 2), (16, 32),        # elbo_rows_mfma_kernel<T, 1, 2>
    (16, 33), (5, 64),       # <T, 1, 4>
    (17, 32), (32, 2),       # <T, 2, 2>
    (17, 33), (32, 64),      # <T, 2, 4>: fp64 at (32, 64) is the form's largest LDS footprint
    (16, 65), (32, 65),      # elbo_rows_kernel<T, true>
    (33, 64), (33, 65),      # elbo_rows_kernel<T, false>
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,V", SWEEP)
def test_rows_dispatch_boundaries(K, V, dtype):
    # N = 37 * 9 = 333: 21 row groups, the last with 13 rows (ragged), 6 matrix-core workgroups / 3 one-thread-per-row blocks
    m, eps = _loud_oracle(K, V, 37, 9, dtype)
    assert m.N % 16 != 0 and (m.N + 63) // 64 > 1
    t = TOL[dtype]
    eng = engine_from_oracle(m)
    loss, rows, grads = _step(eng, m, eps)
    loss_ref, g_ref, aux = _check_vs_reference(m, eps, eng.last_jitter_level, loss, rows, grads, t)
    # the data are loud: the clamped topic dominates the softmax on most rows ...
    if K > 1:
        assert (aux["theta"].argmax(0) == K - 1).mean() > 0.6
    # ... and counting the last row twice moves the result far outside the tolerances the kernel is held to
    loss_dup, g_dup, _ = _aux(m, eps, eng.last_jitter_level, n_global=m.N, dup_last=True)
    d_loss = abs(loss_dup - loss_ref) / abs(loss_ref)
    d_phi = relerr(g_dup["phi_unc"], g_ref["phi_unc"])
    assert d_loss > 10 * t["loss"] or d_phi > 10 * t["g"], (d_loss, d_phi)


@pytest.mark.parametrize("K,V", [(16, 32), (16, 64), (32, 32), (32, 64)])
def test_rows_grid_stride(K, V):
    """More row groups than one sweep of the capped grid (1024 workgroups x 4 waves): N = 331 * 211 = 69 841 is 4366 groups, the last
    ragged, so the grid-stride loop and its one-group-ahead prefetch run past the first sweep."""
    dtype = torch.float32
    m, eps = _loud_oracle(K, V, 331, 211, dtype)
    assert (m.N + 15) // 16 > 1024 * 4 and m.N % 16 != 0
    eng = engine_from_oracle(m)
    loss, rows, grads = _step(eng, m, eps)
    _check_vs_reference(m, eps, eng.last_jitter_level, loss, rows, grads, TOL[dtype])


def _ctx_bytes(n_cap, M, K, V, dtype):
    """Device bytes of an Engine with this capacity, from the buffers of gdrf_ctx_create_ex that grow with n_cap (K_nm, W, Wbar, the
    partial row norms, q, asum, the five (K, ldk) arrays and, in fp32, the scaled vbar copy and the dK_nm pieces the first step
    allocates), one (K, ldk) workspace copy the test reads through, and 1 GB for everything of fixed size."""
    Mp = (M + 31) // 32 * 32
    ldk = (n_cap + 3) // 4 * 4
    esz = 8 if dtype == torch.float64 else 4
    b = n_cap * Mp * 8 + 2 * n_cap * Mp * esz + ((Mp + 63) // 64 + 2) * ldk * esz + 5 * K * ldk * esz
    if esz == 4:
        b += K * ((n_cap + 63) // 64 * 64) * 4 + 2 * n_cap * Mp * 2
    return b + K * ldk * esz + (1 << 30)


@pytest.mark.parametrize("dtype,n_cap", [(torch.float64, 17_500_000), (torch.float32, 35_000_000)])
def test_rows_offsets_past_4gib(dtype, n_cap):
    """K = 32, V = 64, M = 12 with a capacity whose (K, ldk) arrays put topic 31 more than 4 GiB past topic 0
    (31 * ldk * sizeof(T) = 4.34e9 bytes) while the step itself has ~3000 rows: the row kernel must not address them by 32-bit offsets."""
    K, V = 32, 64
    m, eps = _loud_oracle(K, V, 61, 49, dtype)
    esz = 8 if dtype == torch.float64 else 4
    assert (K - 1) * ((n_cap + 3) // 4 * 4) * esz >= 1 << 32
    need = _ctx_bytes(n_cap, m.M, K, V, dtype)
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        pytest.skip(f"needs ~{need / 1e9:.1f} GB of device memory, {free / 1e9:.1f} GB free")
    t = TOL[dtype]
    eng = engine_from_oracle(m, n_cap=n_cap)
    loss, rows, grads = _step(eng, m, eps)
    level = eng.last_jitter_level
    del eng                                   # free the large context before the next one
    gc.collect()
    torch.cuda.empty_cache()
    _check_vs_reference(m, eps, level, loss, rows, grads, t)
    # the same step on an engine with n_cap = n (small offsets): fp64 agrees to round-off; fp32 evaluates its row terms with other
    # (hardware) transcendentals in the matrix-core form and is held to the parity table
    small = engine_from_oracle(m)
    loss_s, rows_s, grads_s = _step(small, m, eps)
    assert small.last_jitter_level == level
    del small
    gc.collect()
    torch.cuda.empty_cache()
    if dtype == torch.float64:
        rep = {name: relerr(rows[name], rows_s[name]) for name in rows}
        rep.update({"g_" + name: relerr(grads[name], grads_s[name]) for name in grads})
        rep["loss"] = abs(loss - loss_s) / abs(loss_s)
        assert max(rep.values()) < 1e-12, rep
    else:
        _assert_close(loss, rows, grads, loss_s, rows_s, grads_s, t)
