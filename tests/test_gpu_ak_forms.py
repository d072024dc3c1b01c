"""GPU: the two shipped forms of the A_k = W^T diag(vbar_k) W kernel (csrc/gemm_tn_topics.h: two waves per SIMD; csrc/gemm_tn_topics1.h:
one wave per SIMD with 128 rows per wave, inline-asm MFMAs, AGPR accumulators, 3-deep LDS-DMA ring) and the tt kernel, each against the
fp64 product of the engine's OWN float32 inputs, on shapes that reach their edges: rows that are no multiple of the 64-row chunk, splits
with no rows at all, more topics than one accumulator group holds (K = 11, 12 -> groups of 10 + 1, 10 + 2), fewer (K = 3 .. 5), a padded
inducing count (M = 100 -> Mp = 128), an inducing count that is no multiple of the tiles (M = 480), and the headline's M = 512.  K alone
selects the form: the two-wave form when more than 40 % of the topic slots of the one-wave form's 10-topic groups would be empty (K <= 5,
K = 11), the one-wave form otherwise."""
import numpy as np
import pytest
import torch

from tests._util import dev, engine_from_oracle, make_oracle, relerr

pytestmark = pytest.mark.gpu

SHAPES = {
    # one-wave form
    "m256_k10_ragged_rows": dict(kind="rbf", W=41, H=25, V=20, K=10, n_points=(16, 16), lengthscale=0.08),       # N = 1025
    "m100_k12_two_groups": dict(kind="matern52", W=40, H=25, V=12, K=12, n_points=(10, 10), lengthscale=0.12),   # Mp = 128
    "m480_k10_partial_tiles": dict(kind="rbf", W=50, H=40, V=20, K=10, n_points=(24, 20), lengthscale=0.1),       # Mp = 480: the last 128 / 64 tiles are partial
    # two-wave form
    "m512_k3": dict(kind="rbf", W=60, H=50, V=20, K=3, n_points=(32, 16), lengthscale=0.1),
    "m256_k4_ragged_rows": dict(kind="rbf", W=41, H=25, V=20, K=4, n_points=(16, 16), lengthscale=0.08),         # N = 1025
    "m100_k5_padded": dict(kind="matern52", W=40, H=25, V=12, K=5, n_points=(10, 10), lengthscale=0.12),          # Mp = 128
    "m480_k11_partial_tiles": dict(kind="rbf", W=50, H=40, V=20, K=11, n_points=(24, 20), lengthscale=0.1),       # two topic groups, N = 2000
}


def _run(m, eps):
    eng = engine_from_oracle(m, mfma_mode="f16x3", store_t=False)
    xs, ws, e = dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng)
    eng.loss_and_grads(xs, ws, e)
    torch.cuda.synchronize()
    n = m.N
    Wm = eng.workspace("W", n).cpu().double().numpy()
    vbar = eng.workspace("vbar", n).cpu().double().numpy()
    S = eng.workspace("S").cpu().double().numpy()
    Mp, lay = (m.M + 31) // 32 * 32, eng.red_layout
    A = eng.red_T[lay["A"]:lay["A"] + m.K * Mp * Mp].view(m.K, Mp, Mp)[:, :m.M, :m.M].cpu().double().numpy()
    tt = eng.workspace("tt", n).cpu().double().numpy()
    A_ref = np.stack([Wm.T @ (vbar[k][:, None] * Wm) for k in range(m.K)])
    tt_ref = np.stack([((Wm @ S[k]) ** 2).sum(1) for k in range(m.K)])
    # second call on the same engine: bit-identical (fixed accumulation order)
    eng.loss_and_grads(xs, ws, e)
    torch.cuda.synchronize()
    A2 = eng.red_T[lay["A"]:lay["A"] + m.K * Mp * Mp].view(m.K, Mp, Mp)[:, :m.M, :m.M].cpu().double().numpy()
    assert np.array_equal(A, A2), (float(np.abs(A - A2).max()), float(np.abs(A).max()))
    return dict(A=np.tril(A), A_ref=np.tril(A_ref), tt=tt, tt_ref=tt_ref)


@pytest.mark.parametrize("name", list(SHAPES))
def test_ak_kernel_forms_agree_with_the_fp64_product(name):
    m, eps = make_oracle(dtype=torch.float32, jitter=1e-4, **SHAPES[name])
    r = _run(m, eps)
    err_a, err_t = relerr(r["A"], r["A_ref"]), relerr(r["tt"], r["tt_ref"])
    print(name, "vs the fp64 product of the same inputs: A_k %.2e, tt %.2e" % (err_a, err_t))
    assert err_a < 2e-6, (name, err_a)                       # 22-bit arithmetic: the split forms measure 2 - 5e-7 here
    assert err_t < 2e-6, (name, err_t)
