"""GPU: the one-wave-per-SIMD form of the f16x3 tt contraction (csrc/gemm_split.h, fwd_t_f16_w1_kernel: two topics per wave, the
accumulators in AGPRs, S_k^T fragments from L2 straight into registers, the W image double-buffered in LDS, one barrier per 64-deep reduction
block; K / 4 * 4 topics run on its quad geometry - one row tile x four topics per workgroup -, the K % 4 left over on its pair geometry - two
row tiles x two topics) against the fp64 value ((W S_k)^2).sum(1) of the engine's OWN float32 W and S, so that only the kernel's arithmetic differs.  The host
takes the form under the gate of the W-bar form of the same geometry (row-tile pairs x column tiles > 32, Mp % 64 == 0, 2 <= K <= 16); every
case asserts that it ran.  The bound is the one tests/test_gpu_parity.py::test_split_modes_against_fp64_product_of_the_same_inputs states for
tt: the native f32 MFMA engine on the same inputs below 2e-6, the new form below 1.5 x that + 1e-7, relative to max |tt|.  The shapes are
those of tests/test_gpu_wbar_w1.py: the smallest at which the form is selected and each edge exists."""
import numpy as np
import pytest
import torch

from tests._util import dev, engine_from_oracle, make_oracle, relerr

pytestmark = pytest.mark.gpu

SHAPES = {
    # the headline's tile structure (4 column tiles, 8 + 6 + 4 + 2 reduction blocks; two quad groups, then one pair); 19 row tiles: the last
    # one is ragged (96 rows), the pair geometry's last second tile lies wholly past the end
    "m512_k10_ragged_last_pair": dict(W=60, H=40, K=10, n_points=(32, 16), lengthscale=0.06),
    # one column tile, ONE reduction block, one topic pair (pair geometry only): column half 1 lies wholly past Mp, sits out its only block
    # and folds nothing
    "m64_k2_single_block": dict(W=130, H=65, K=2, n_points=(8, 8), lengthscale=0.2),
    # Mp = 192: the second column tile is half past the end (its column half 1 never multiplies); K = 3: pair geometry, two pairs in one L2
    # group, the last pair holds one topic twice
    "m192_k3_partial_column_tile": dict(W=65, H=67, K=3, n_points=(16, 12), lengthscale=0.1),
    # padded inducing count (M = 100 in Mp = 128), the largest K of the gate: four quad groups, no pair launch
    "m100_k16_padded": dict(kind="matern52", W=130, H=65, K=16, n_points=(10, 10), lengthscale=0.12),
    # two column tiles; K = 5: one quad group, then a pair launch of a single topic
    "m256_k5": dict(W=80, H=55, K=5, n_points=(16, 16), lengthscale=0.08),
    # the W pieces' stride n_cap * Mp differs from n * Mp; K = 9: two quad groups and a single topic
    "m256_k9_ncap_twice_n": dict(W=80, H=55, K=9, n_points=(16, 16), lengthscale=0.08, n_cap=8800),
}


def _perturb_wide(m, spread):
    """The construction of tests/test_gpu_parity.py: S_k rows and u_loc scaled by powers of ten drawn per topic / row."""
    g = torch.Generator().manual_seed(77)
    lower = torch.distributions.transform_to(torch.distributions.constraints.lower_cholesky)
    with torch.no_grad():
        K, M = m.params["u_loc"].shape
        rowscale = 10.0 ** (spread * (torch.rand(K, M, 1, generator=g) - 0.5))
        S = lower(m.params["u_scale_tril_unc"].double()) * rowscale.double()
        m.params["u_scale_tril_unc"].copy_(lower.inv(S).to(m.dtype))
        m.params["u_loc"].mul_(10.0 ** (spread * (torch.rand(K, M, generator=g) - 0.5)).to(m.dtype))


def _tt_and_ref(eng, m, xs, ws, e):
    """One step; tt and the fp64 value from the step's own W and S."""
    eng.loss_and_grads(xs, ws, e)
    torch.cuda.synchronize()
    n = m.N
    Wm = eng.workspace("W", n).cpu().double().numpy()
    S = eng.workspace("S").cpu().double().numpy()
    ref = np.stack([((Wm @ S[k]) ** 2).sum(1) for k in range(m.K)])
    return eng.workspace("tt", n).clone().cpu(), ref


def _run(m, eps, n_cap=None):
    err = {}
    for mode in ("f32", "f16x3"):
        eng = engine_from_oracle(m, mfma_mode=mode, store_t=False, n_cap=n_cap)
        xs, ws, e = dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng)
        tt, ref = _tt_and_ref(eng, m, xs, ws, e)
        assert eng.read_out()["chol_failed"] == 0
        err[mode] = relerr(tt.double().numpy(), ref)
        if mode == "f16x3":
            forms = eng.last_forms()
            # topics per L2 group: four on the quad form (K >= 4), else the pair form's two pairs at most
            assert forms["fwd_t"] == "w1" and forms["fwd_t_kg"] == (4 if m.K >= 4 else 2 * min(2, (m.K + 1) // 2)), forms
            # the same step again on the same engine: bit-identical (fixed accumulation order, no atomics)
            tt2, _ = _tt_and_ref(eng, m, xs, ws, e)
            assert torch.equal(tt, tt2), float((tt - tt2).abs().max())
    return err


def _check(name, m, err):
    print(name, "n = %d, tt vs the fp64 product of the same inputs: f32 MFMA %.2e, w1 %.2e" % (m.N, err["f32"], err["f16x3"]))
    assert err["f32"] < 2e-6, err
    assert err["f16x3"] < 1.5 * err["f32"] + 1e-7, err


@pytest.mark.parametrize("name", list(SHAPES))
def test_w1_tt_against_the_fp64_product_of_the_same_inputs(name):
    kw = dict(SHAPES[name])
    n_cap = kw.pop("n_cap", None)
    kw.setdefault("kind", "rbf")
    m, eps = make_oracle(dtype=torch.float32, jitter=1e-4, V=12, **kw)
    _check(name, m, _run(m, eps, n_cap))


def test_w1_tt_with_factors_spread_over_seven_decades():
    m, eps = make_oracle(dtype=torch.float32, jitter=1e-4, V=12, kind="rbf", **SHAPES["m512_k10_ragged_last_pair"])
    _perturb_wide(m, 7.0)
    _check("spread 7.0", m, _run(m, eps))
