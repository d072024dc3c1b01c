"""GPU: the one-wave-per-SIMD form of the f16x3 W-bar contraction (csrc/gemm_split.h, bwd_wbar_f16_w1_kernel: B_k fragments from L2 straight
into registers, the W image double-buffered in LDS, one barrier per 64-deep reduction block) against the fp64 product of the engine's OWN
float32 inputs (W, vbar, locbar, asum, S, u_loc), so that only the kernel's arithmetic differs.  The host takes the form when the reduction is
not sliced (row-tile pairs x column tiles > 32), Mp % 64 == 0 and 2 <= K <= 16; every case asserts that it ran.  The bound is the one
tests/test_gpu_parity.py::test_split_modes_against_fp64_product_of_the_same_inputs holds the k64 form to: 1.5 x the error of the native f32 MFMA
engine on the same inputs + 1e-7, relative to max |W-bar| (at a spread of seven decades inside one block scale: the 1e-5 that test states for
f16x3).  The shapes are the smallest at which the form is selected and each edge exists."""
import pytest
import torch

from tests._util import dev, engine_from_oracle, make_oracle, relerr

pytestmark = pytest.mark.gpu

SHAPES = {
    # the headline's tile structure (4 column tiles, 8 reduction blocks x 10 topics); 19 row tiles: the last pair's first tile is ragged
    # (96 rows), its second lies wholly past the end
    "m512_k10_ragged_last_pair": dict(W=60, H=40, K=10, n_points=(32, 16), lengthscale=0.06),
    # one column tile, ONE reduction block (the W double buffer never advances), the smallest K: 8 requests of the image per phase
    "m64_k2_single_block": dict(W=130, H=65, K=2, n_points=(8, 8), lengthscale=0.2),
    # Mp = 192: the second column tile is half past the end - the column clamps of the B loads, the W tile loads and the store; 3 blocks x 3 topics
    # = 9 phases: the two-phase loop body runs its padding phase with all-zero factors
    "m192_k3_partial_column_tile": dict(W=65, H=67, K=3, n_points=(16, 12), lengthscale=0.1),
    # padded inducing count (col < M in the rank-K term), K = 16: a full 16-topic table, two 8-topic rank-K batches
    "m100_k16_padded": dict(kind="matern52", W=130, H=65, K=16, n_points=(10, 10), lengthscale=0.12),
    # the W pieces' stride n_cap * Mp differs from n * Mp; K = 9: the image's 16 requests go out in 8 phases, the ninth repeats the last two
    # 4 <= K <= 7: the instantiation with four W-image requests per phase (two behind column group 0, two behind group 2), whose literal
    # vmcnt counts differ from the K >= 8 and K <= 3 ones; 4 blocks x 5 topics
    "m256_k5_four_requests_per_phase": dict(W=80, H=55, K=5, n_points=(16, 16), lengthscale=0.08),
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


def _wbar_and_ref(eng, m, xs, ws, e):
    """One step; W-bar, the fp64 product of the step's own inputs, and G^T."""
    eng.loss_and_grads(xs, ws, e)
    torch.cuda.synchronize()
    n = m.N
    Wm = eng.workspace("W", n).cpu().double().numpy()
    vbar = eng.workspace("vbar", n).cpu().double().numpy()
    locbar = eng.workspace("locbar", n).cpu().double().numpy()
    asum = eng.workspace("asum", n).cpu().double().numpy()
    S = eng.workspace("S").cpu().double().numpy()
    U = eng.view("u_loc").cpu().double().numpy()
    ref = locbar.T @ U - 2 * asum[:, None] * Wm
    for k in range(m.K):
        ref += (2 * vbar[k])[:, None] * (Wm @ (S[k] @ S[k].T))
    Mp, lay = (m.M + 31) // 32 * 32, eng.red_layout
    GT = eng.red_T[lay["GT"]:lay["GT"] + Mp * Mp].clone().cpu()
    return eng.workspace("Wbar", n).clone().cpu(), ref, GT


def _run(m, eps, n_cap=None):
    err = {}
    for mode in ("f32", "f16x3"):
        eng = engine_from_oracle(m, mfma_mode=mode, store_t=False, n_cap=n_cap)
        xs, ws, e = dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng)
        wbar, ref, GT = _wbar_and_ref(eng, m, xs, ws, e)
        assert eng.read_out()["chol_failed"] == 0
        err[mode] = relerr(wbar.double().numpy(), ref)
        if mode == "f16x3":
            forms = eng.last_forms()
            assert forms["wbar"] == "w1" and forms["wbar_nslice"] == 1, forms
            # the same step again on the same engine: bit-identical (fixed accumulation order, no atomics but the integer maximum)
            wbar2, _, GT2 = _wbar_and_ref(eng, m, xs, ws, e)
            assert torch.equal(wbar, wbar2), float((wbar - wbar2).abs().max())
            assert torch.equal(GT, GT2), float((GT - GT2).abs().max())
    return err


@pytest.mark.parametrize("name", list(SHAPES))
def test_w1_wbar_against_the_fp64_product_of_the_same_inputs(name):
    kw = dict(SHAPES[name])
    n_cap = kw.pop("n_cap", None)
    kw.setdefault("kind", "rbf")
    m, eps = make_oracle(dtype=torch.float32, jitter=1e-4, V=12, **kw)
    err = _run(m, eps, n_cap)
    print(name, "n = %d, W-bar vs the fp64 product of the same inputs: f32 MFMA %.2e, w1 %.2e" % (m.N, err["f32"], err["f16x3"]))
    assert err["f32"] < 2e-5, err
    assert err["f16x3"] < 1.5 * err["f32"] + 1e-7, err


def test_w1_wbar_with_factors_spread_over_seven_decades():
    m, eps = make_oracle(dtype=torch.float32, jitter=1e-4, V=12, kind="rbf", **SHAPES["m512_k10_ragged_last_pair"])
    _perturb_wide(m, 7.0)
    err = _run(m, eps)
    print("spread 7.0: f32 MFMA %.2e, w1 %.2e" % (err["f32"], err["f16x3"]))
    assert err["f16x3"] < 1e-5, err
