"""GPU tests of the routing of the two side paths: the custom-link step (gdrf_step_local_link) and the two-point step of a non-unit
world (gdrf_step_local2).

Both run on the V-free kernels of csrc/rows_lds.h around the streamed (or sparse) vocabulary kernel in EVERY row form: row form 0
("auto") selects the LDS kernels of gdrf_step_local and gdrf_predict only.  So for these two entry points "auto" and "streamed" launch
the same kernels on the same grid (the grid depends on n_cap, K and V alone) and agree bit for bit, and neither has a vocabulary ceiling:
the shape whose "too large" tests/test_gpu_round2.py pins for gdrf_step_local runs here in row form 0."""
import numpy as np
import pytest
import torch

from oracle.gdrf_oracle import RefShapedGDRF
from tests._util import dev, relerr
from tests.test_gpu_round2 import _LINKS, WORLD, _world_oracle
from tests.test_gpu_vocab_stream import LOSS_TOL_VS_TORCH, _engine

pytestmark = pytest.mark.gpu


def _perturb(m, g):
    with torch.no_grad():
        m.params["u_loc"].add_(0.3 * torch.randn(m.params["u_loc"].shape, generator=g, dtype=torch.float64))
        m.params["phi_unc"].add_(0.5 * torch.randn(m.params["phi_unc"].shape, generator=g, dtype=torch.float64))


def _link_oracle(link, V, K=4, W=17, H=9, n_points=(4, 3), jitter=1e-6, whiten=True):
    from gdrf_amd.data import synth_circles
    xs, ws, _ = synth_circles(W, H, V, K, seed=4)
    m = RefShapedGDRF(xs, ws, kind="rbf", K=K, n_points=n_points, lengthscale=0.2, dtype=torch.float64, jitter=jitter,
                      link_function=_LINKS[link], optimizer="adam", lr=1e-2, whiten=whiten)
    g = torch.Generator().manual_seed(21)
    _perturb(m, g)
    return m, torch.randn(K, m.N, generator=g, dtype=torch.float64)


def _link_step(m, eps, link, rows_form, dtype):
    eng = _engine(m, rows_form=rows_form, dtype=dtype)
    eng.link_function = _LINKS[link]
    eng.loss_and_grads(dev(m.xs, eng), dev(m.ws, eng, torch.int32), dev(eps, eng))
    return eng, _result(eng)


def _world_step(m, eps, xs_w, rows_form, dtype):
    eng = _engine(m, rows_form=rows_form, dtype=dtype)
    xs_m = m.scale(xs_w)
    eng.loss_and_grads(dev(xs_m, eng), dev(m.ws, eng, torch.int32), dev(eps, eng), xs_guide=dev(m.scale(xs_m), eng),
                       force_level=m.last_jitter_level)
    return eng, _result(eng)


def _result(eng):
    out = eng.read_out()
    assert out["chol_failed"] == 0
    return out["loss"], {name: v.cpu().numpy().copy() for name, v in eng.named_views(eng.grads).items()}


def _assert_identical(a, b):
    assert np.isfinite(a[0]) and a[0] == b[0], (a[0], b[0])
    for name in a[1]:
        assert np.isfinite(a[1][name]).all() and np.array_equal(a[1][name], b[1][name]), name


def _assert_oracle(eng, res, loss_ref, grads_ref):
    assert abs(res[0] - loss_ref) <= LOSS_TOL_VS_TORCH * abs(loss_ref), (res[0], loss_ref)
    for name in eng.PARAM_NAMES:
        assert relerr(res[1][name], grads_ref[name].numpy()) < 1e-7, name


# ---- 1. row forms 0 and 1 are one route for the two side paths: K = 4, V = 13, N = 17 x 9 (link) and the two-point shape of round 2
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("link", ["sigmoid", "tempered_softmax"])          # theta that does not / does sum to one over the topics
def test_link_step_is_the_same_in_both_row_forms(link, dtype):
    m, eps = _link_oracle(link, V=13, jitter=1e-6 if dtype == torch.float64 else 1e-4)
    _, a = _link_step(m, eps, link, "auto", dtype)
    _, b = _link_step(m, eps, link, "streamed", dtype)
    _assert_identical(a, b)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_two_point_step_is_the_same_in_both_row_forms(dtype):
    m, eps, xs_w = _world_oracle(torch.float64)
    m.loss_and_grads(eps)                    # fixes the jitter level both engines are forced to
    _, a = _world_step(m, eps, xs_w, "auto", dtype)
    _, b = _world_step(m, eps, xs_w, "streamed", dtype)
    _assert_identical(a, b)


# ---- 2. no vocabulary ceiling in row form 0: K = 5, V = 2500 in fp64, where gdrf_step_local fails with "too large"
def test_link_step_past_the_lds_ceiling_in_row_form_0():
    m, eps = _link_oracle("sigmoid", V=2500, K=5, W=6, H=5, n_points=(3, 2))
    eng, res = _link_step(m, eps, "sigmoid", "auto", torch.float64)
    m.force_jitter_level = eng.last_jitter_level
    _assert_oracle(eng, res, *m.loss_and_grads(eps))


def test_two_point_step_past_the_lds_ceiling_in_row_form_0():
    from gdrf_amd.data import synth_circles
    xs, ws, _ = synth_circles(6, 5, 2500, 5, seed=4)
    lower = torch.tensor([w[0] for w in WORLD], dtype=torch.float64)
    delta = torch.tensor([w[1] - w[0] for w in WORLD], dtype=torch.float64)
    xs_w = torch.from_numpy(xs).double() * delta + lower
    m = RefShapedGDRF(xs_w, ws, kind="rbf", K=5, n_points=(3, 2), lengthscale=0.3, dtype=torch.float64, jitter=1e-6, world=WORLD,
                      guide_rescale=True, optimizer="adam", lr=1e-2)
    g = torch.Generator().manual_seed(5)
    _perturb(m, g)
    eps = torch.randn(5, m.N, generator=g, dtype=torch.float64)
    ref = m.loss_and_grads(eps)
    eng, res = _world_step(m, eps, xs_w, "auto", torch.float64)
    _assert_oracle(eng, res, *ref)


# ---- 3. unwhitened contexts: the backward of both side paths runs in a call of its own, behind a forward that is not the one the
# transforms ran in front of, and has to read u' = L^-1 u (not the parameter u) for Wbar.  K = 4, V = 13, N = 17 x 9, M = 12 (Mp padded)
def _perturb_scale(m, g):
    with torch.no_grad():
        m.params["u_scale_tril_unc"].add_(0.1 * torch.randn(m.params["u_scale_tril_unc"].shape, generator=g, dtype=torch.float64).tril())


def test_link_step_unwhitened():
    m, eps = _link_oracle("sigmoid", V=13, whiten=False)
    _perturb_scale(m, torch.Generator().manual_seed(22))
    eng, res = _link_step(m, eps, "sigmoid", "auto", torch.float64)
    m.force_jitter_level = eng.last_jitter_level
    _assert_oracle(eng, res, *m.loss_and_grads(eps))


def test_two_point_step_unwhitened():
    from gdrf_amd.data import synth_circles
    xs, ws, _ = synth_circles(17, 9, 13, 4, seed=4)
    lower = torch.tensor([w[0] for w in WORLD], dtype=torch.float64)
    delta = torch.tensor([w[1] - w[0] for w in WORLD], dtype=torch.float64)
    xs_w = torch.from_numpy(xs).double() * delta + lower
    m = RefShapedGDRF(xs_w, ws, kind="rbf", K=4, n_points=(4, 3), lengthscale=0.3, dtype=torch.float64, jitter=1e-6, world=WORLD,
                      guide_rescale=True, optimizer="adam", lr=1e-2, whiten=False)
    g = torch.Generator().manual_seed(5)
    _perturb(m, g)
    _perturb_scale(m, g)
    eps = torch.randn(4, m.N, generator=g, dtype=torch.float64)
    ref = m.loss_and_grads(eps)
    eng, res = _world_step(m, eps, xs_w, "auto", torch.float64)
    _assert_oracle(eng, res, *ref)
