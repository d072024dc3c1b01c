"""GPU: step_finish's gradients at K = 1, where every batched M x M product is a single one and takes the split-K form of Impl::mm_nt
(csrc/forms.h: mm_plan) wherever a single product does.  In the whitened form Sbar_k = 2 A_k S_k runs on the side stream BESIDE the
Cholesky-backward chain, whose products go through the context's one slab buffer: until mm_plan read `beside_chain`, both wrote that buffer
at the same time at K = 1 (Mp a multiple of 256 in float, of 128 from 256 in double), which left NaN and 1e35-sized entries in the
u_scale_tril_unc block of `grads` that changed from run to run, and could damage the chain's HT just as well.

a. every gradient block against fp64 autograd of the oracle at Mp = 224 (no product splits), 256, 384 (the double ones split) and 512, float
   and double arrays, whitened and unwhitened, with K = 2 at Mp = 256 as the control whose Sbar product never splits;
b. the u_scale_tril_unc block against the fp64 product of the engine's OWN A_k and S_k (and L^-1, unwhitened), globally and per 128 x 128 tile;
c. a K = 1 engine built after a K = 8 engine ran in the process: finite, and bit-identical over two evaluations.
Every case asserts the forms it targets through Engine.last_forms() (mm_chain, mm_sbar)."""
import functools

import numpy as np
import pytest
import torch

from tests._util import dev, engine_from_oracle, make_oracle, relerr
from tests.test_gpu_round3 import BLOCKS, LOSS_TOL_FP64, REGIMES, _all_block_errors, _assert_fp32, _fp32_valued
from tests.test_gpu_topic_forms import GLOBAL, TILE, TILE_TOL, _tile_err

pytestmark = pytest.mark.gpu

GRIDS = {224: (16, 14), 256: (16, 16), 384: (24, 16), 512: (32, 16)}        # Mp (= M: all multiples of 32) -> n_points
# The whitened cases run at lengthscale 0.12: cond(K_uu + jitter) = 1.6e7 (Mp = 224) to 3.8e7 (Mp = 512), the jitter's floor.  The unwhitened
# gradients are chained through S' = L^-1 S and Sbar = L^-T Sbar', so round-off reaches them times cond(K_uu): at 0.12 the fp64 engine and fp64
# autograd - each with that error - differ by up to 2.4e-6 (log_variance) and 5.4e-7 (u_scale_tril_unc) whether or not a product splits (Mp = 224:
# none does; K = 2 as well), the float engine by up to 1.0 and 0.2, and the product test b differs from its fp64 reference by 7e-10 in double and
# 0.11 in float: the same factor ~1e6 - 1e7 times the unit round-off of either type, which is conditioning and not a defect.  A WIDER
# lengthscale only worsens it (cond is at the jitter's floor already); the unwhitened cases therefore take 0.03, where cond(K_uu) is 1.6
# (Mp = 224), 2.0, 7.2 and 48 (Mp = 512) and L^-1 still has Mp / 8-deep off-diagonal structure for the split products to lose.
LENGTHSCALE = {True: 0.12, False: 0.03}         # by whiten


@functools.lru_cache(maxsize=None)
def _oracle(Mp, K, whiten, fp32_valued):
    """(oracle, eps), built once per case and shared; the tests only set its force_jitter_level, which every use sets anew."""
    m, eps = make_oracle(kind="rbf", W=25, H=16, V=12, K=K, n_points=GRIDS[Mp], dtype=torch.float64, jitter=1e-6,
                         lengthscale=LENGTHSCALE[whiten], whiten=whiten, **REGIMES["trained"])
    return (_fp32_valued(m) if fp32_valued else m), eps


def _want_forms(Mp, K, arrays, whiten):
    """mm_chain: single products in the solve precision (double unless pure_fp32) - eight slices of whole 16-deep (double) or 32-deep (float)
    chunks from Mp = 256.  mm_sbar: K products in the arrays' precision - split only as a single product (K = 1) that runs alone (unwhitened)."""
    splits = lambda esz: Mp >= 256 and (Mp // 8) % (32 if esz == 4 else 16) == 0
    esz, ssz = {"f32": (4, 8), "f64": (8, 8), "pure": (4, 4)}[arrays]
    return dict(mm_chain="split8" if splits(ssz) else "direct", mm_sbar="split8" if K == 1 and not whiten and splits(esz) else "direct")


def _block_errors(m, eps, dtype):
    """_all_block_errors, with the u_loc block of a one-topic model measured on a scale that exists.  The softmax link of a single topic is
    constant, so d loss / d u_loc is identically zero at K = 1: the engine's block is exactly 0, the oracle's is its own round-off (8.7e-19 to
    3.3e-18 at these shapes), and an error relative to THAT is 1 whatever the engine does.  There the block's error is taken relative to the larger of the two variational blocks' max |ref|,
    that is u_scale_tril_unc's (4.6e-3 to 8.8e-3): the same bound then holds u_loc's absolute error to what it holds u_scale_tril_unc's."""
    lvl, errs, eng = _all_block_errors(m, eps, dtype)
    if m.K == 1:
        _, ref = m.loss_and_grads(eps)                 # at the level _all_block_errors forced
        got = eng.view("u_loc", eng.grads).cpu().double().numpy()
        ref_u, ref_s = ref["u_loc"].double().numpy(), ref["u_scale_tril_unc"].double().numpy()
        print("   K = 1: max |u_loc gradient| got %.2e, oracle %.2e; max |ref| of u_scale_tril_unc %.2e" % (np.abs(got).max(), np.abs(ref_u).max(), np.abs(ref_s).max()))
        errs["u_loc"] = float(np.abs(got - ref_u).max() / max(np.abs(ref_u).max(), np.abs(ref_s).max()))
    return lvl, errs, eng


def _assert_blocks(errs, dtype):
    if dtype == torch.float32:
        _assert_fp32(errs, "trained")
    else:
        assert errs["loss"] < LOSS_TOL_FP64
        for name in BLOCKS:
            assert errs[name] < 1e-7, (name, errs)


# ---- a. every gradient block against fp64 autograd -----------------------------------------------------------------------------------------

A_CASES = [(Mp, 1) for Mp in GRIDS] + [(256, 2)]


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("Mp,K", A_CASES, ids=["Mp%d_K%d" % c for c in A_CASES])
def test_all_gradient_blocks_at_one_topic(Mp, K, dtype, whiten):
    m, eps = _oracle(Mp, K, whiten, dtype == torch.float32)
    lvl, errs, eng = _block_errors(m, eps, dtype)
    seen = eng.last_forms()
    print("Mp", Mp, "K", K, dtype, "whiten", whiten, "level", lvl, {k: seen.get(k) for k in ("mm_chain", "mm_sbar")}, {k: f"{v:.2e}" for k, v in errs.items()})
    assert m.M == Mp and eng.whiten == whiten
    if dtype == torch.float32:
        assert eng.mfma_mode == "f16x3"
    want = _want_forms(Mp, K, "f32" if dtype == torch.float32 else "f64", whiten)
    assert {k: seen.get(k) for k in want} == want, seen
    _assert_blocks(errs, dtype)


# ---- b. the S-bar product against the fp64 product of the engine's own inputs ----------------------------------------------------------------

def _grad_s_ref(eng, n):
    """d loss / d u_scale_tril_unc in fp64 from what the engine itself holds after a step: Sbar = 2 A S (A_k: the lower triangle of red_T's
    block, mirrored; S: workspace "S" - unwhitened that is S' = L^-1 S, and Sbar = L^-T (2 A S')), then the lower_cholesky transform:
    Sbar below the diagonal, Sbar_ii S_ii on it (S_ii = exp of the parameter: the unwhitened S' has another diagonal), times -1 / n."""
    K, M = eng.K, eng.M
    Mp, lay = (M + 31) // 32 * 32, eng.red_layout
    low = np.tril(eng.red_T.cpu().double().numpy()[lay["A"]:lay["A"] + K * Mp * Mp].reshape(K, Mp, Mp)[:, :M, :M])
    A = low + np.transpose(np.tril(low, -1), (0, 2, 1))
    S = eng.workspace("S").cpu().double().numpy()
    Sbar = 2.0 * A @ S
    if not eng.whiten:
        Sbar = eng.workspace("Linv").cpu().double().numpy().T @ Sbar
    diag = np.exp(np.diagonal(eng.view("u_scale_tril_unc").cpu().double().numpy(), axis1=1, axis2=2))
    g = np.tril(Sbar, -1)
    g[:, np.arange(M), np.arange(M)] = np.diagonal(Sbar, axis1=1, axis2=2) * diag
    return -g / n


B_CASES = [(256, "f32", True), (512, "f32", True), (256, "f64", True), (512, "f64", True), (256, "pure", True), (512, "pure", True),
           (256, "f32", False), (256, "f64", False)]


@pytest.mark.parametrize("Mp,arrays,whiten", B_CASES, ids=["Mp%d_%s_%s" % (c[0], c[1], "whitened" if c[2] else "unwhitened") for c in B_CASES])
def test_scale_tril_gradient_against_the_fp64_product_of_the_engine_inputs(Mp, arrays, whiten):
    m, eps = _oracle(Mp, 1, whiten, arrays != "f64")
    dtype = torch.float64 if arrays == "f64" else torch.float32
    eng = engine_from_oracle(m, dtype=dtype, pure_fp32=arrays == "pure")
    eng.loss_and_grads(dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng))
    assert eng.read_out()["chol_failed"] == 0
    seen = eng.last_forms()
    got = eng.view("u_scale_tril_unc", eng.grads).cpu().double().numpy()
    ref = _grad_s_ref(eng, m.N)
    g, t = relerr(got, ref), _tile_err(got, ref, TILE, TILE)
    bound = GLOBAL["f64" if arrays == "f64" else "f32"]["A"]
    print("Mp", Mp, arrays, "whiten", whiten, "level", eng.last_jitter_level, {k: seen.get(k) for k in ("mm_chain", "mm_sbar")},
          "global %.2e (bound %.0e)  per tile %.2e (bound %.0e)" % (g, bound, t, TILE_TOL))
    want = _want_forms(Mp, 1, arrays, whiten)
    assert {k: seen.get(k) for k in want} == want, seen
    assert np.isfinite(got).all()
    assert g < bound and t < TILE_TOL, (g, t)


# ---- c. after another engine ran in the process, and twice ---------------------------------------------------------------------------------

def test_one_topic_gradients_after_another_engine_ran_and_twice():
    m8, eps8 = _oracle(256, 8, True, True)
    eng8 = engine_from_oracle(m8, dtype=torch.float32)
    eng8.loss_and_grads(dev(m8.xs, eng8), dev(m8.ws, eng8, torch.int32), dev(eps8, eng8))
    assert eng8.read_out()["chol_failed"] == 0 and eng8.last_forms()["mm_sbar"] == "direct"
    m, eps = _oracle(256, 1, True, True)
    lvl, errs, eng = _block_errors(m, eps, torch.float32)
    first = eng.grads.cpu().numpy().copy()
    eng.loss_and_grads(dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), force_level=lvl)
    assert eng.read_out()["chol_failed"] == 0
    second = eng.grads.cpu().numpy()
    print("K = 1 after K = 8: level", lvl, eng.last_forms(), {k: f"{v:.2e}" for k, v in errs.items()})
    assert eng.last_forms()["mm_chain"] == "split8" and eng.last_forms()["mm_sbar"] == "direct"
    assert np.isfinite(first).all() and np.isfinite(second).all()
    assert np.array_equal(first, second), float(np.abs(first - second).max())
    _assert_blocks(errs, torch.float32)
