"""Every topic-count form of the f32 step kernels up to K = 128, each stage against the fp64 product of the engine's OWN inputs (W, S_k,
vbar, locbar, asum, u_loc), so that only the kernel's arithmetic differs.  The host picks the forms of W-bar, tt, A_k, loc and ubar from K,
Mp and n (csrc/api.hip); Engine.last_forms() reports what the step launched, and every case asserts the form it targets.

Two measures per output: max |err| / max |ref| over the whole array, and the same ratio inside every 128-row x 128-column tile (per topic
for tt, loc, A_k and ubar), which catches a tile, a reduction slice or a topic that was dropped, doubled or clamped even when it is small.
The data make such faults loud: topic K-1 (the clamped / last-group topic) carries the largest u_k and S_k, the rows of the last, ragged
row tile 20x the counts, and a wide lengthscale keeps every tile's magnitude comparable.  The CPU tests at the end check that these
measures see each simulated fault."""
import numpy as np
import pytest
import torch

from tests._util import dev, make_oracle, relerr

TILE = 128
TILE_TOL = 1e-4            # per tile / per topic, every mode.  Measured on MI355X: at most 1.5e-6 (split), 1.2e-6 (f32), 2.5e-15 (f64)
# global bounds by arithmetic: the split modes are held to what test_gpu_ak_forms / test_gpu_parity hold them to; the native f32 MFMA
# kernels to test_split_modes_against_fp64_product_of_the_same_inputs' bounds; fp64 to round-off.  Largest measured over the cases on
# MI355X - split: Wbar 9.4e-7 (K = 1), tt 6.4e-7, A_k 1.9e-7, G^T 1.3e-7, loc 9.6e-7, ubar 2.7e-7; f32: Wbar 3.8e-7, tt 1.2e-6, A_k 4.0e-7,
# G^T 2.8e-7, loc 9.0e-7, ubar 1.3e-7; f64: 2.1e-15
GLOBAL = {"split": dict(Wbar=2e-6, tt=2e-6, A=2e-6, GT=2e-6, loc=2e-6, ubar=2e-6),
          "f32": dict(Wbar=2e-5, tt=2e-6, A=2e-5, GT=2e-5, loc=2e-6, ubar=2e-6),
          "f64": dict(Wbar=1e-12, tt=1e-12, A=1e-12, GT=1e-12, loc=1e-12, ubar=1e-12)}


def _inputs(K, M, n, V=12, seed=0):
    """Inducing grid, rows, counts and unconstrained parameters (numpy, fp64)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(M)))
    g = (np.arange(side) + 0.5) / side
    Z = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)[:M]
    ws = rng.integers(0, 6, size=(n, V))
    ws[(n - 1) // TILE * TILE:] *= 20
    u = 0.3 * rng.standard_normal((K, M))
    u[K - 1] *= 4
    s = np.tril(0.02 * rng.standard_normal((K, M, M)), -1)
    s[:, np.arange(M), np.arange(M)] = np.log(0.3)
    s[K - 1, np.arange(M), np.arange(M)] = np.log(0.9)
    return dict(Z=Z, X=rng.random((n, 2)), ws=ws.astype(np.int32), eps=rng.standard_normal((K, n)), u_loc=u, u_scale_tril_unc=s,
                phi_unc=0.5 * rng.standard_normal((K, V)))


def _engine(d, n_cap, dtype, **kw):
    from gdrf_amd.engine import Engine
    (K, M), V = d["u_loc"].shape, d["ws"].shape[1]
    eng = Engine(n_cap, M, K, V, 2, dtype=dtype, kernel="matern52", jitter=1e-4, process_group=None, **kw)
    eng.set_inducing_points(torch.from_numpy(d["Z"]))
    eng.set_dirichlet(torch.ones(K, V, dtype=torch.float64))
    vals = dict(log_lengthscale=np.log(0.3), log_variance=0.0, log_noise=np.log(0.5))
    vals.update({k: d[k] for k in ("u_loc", "u_scale_tril_unc", "phi_unc")})
    for name, v in vals.items():
        eng.view(name).copy_(torch.as_tensor(v, dtype=torch.float64).to(dtype))
    return eng


def _step(eng, d):
    n = d["X"].shape[0]
    eng.loss_and_grads(dev(d["X"], eng), dev(d["ws"], eng, torch.int32), dev(d["eps"], eng))
    assert eng.read_out()["chol_failed"] == 0
    K, M = eng.K, eng.M
    Mp, lay = (M + 31) // 32 * 32, eng.red_layout
    red = eng.red_T.cpu().double().numpy()
    r = {name: eng.workspace(name, n).cpu().double().numpy() for name in ("W", "Wbar", "vbar", "locbar", "asum", "tt", "loc")}
    r["S"] = eng.workspace("S").cpu().double().numpy()
    r["U"] = eng.view("u_loc").cpu().double().numpy()
    r["A"] = np.tril(red[lay["A"]:lay["A"] + K * Mp * Mp].reshape(K, Mp, Mp)[:, :M, :M])
    r["GT"] = red[lay["GT"]:lay["GT"] + Mp * Mp].reshape(Mp, Mp)[:M, :M]
    r["ubar"] = red[lay["ubar"]:lay["ubar"] + K * Mp].reshape(K, Mp)[:, :M]
    r["grads"] = eng.grads.cpu().numpy().copy()        # every block, in the arrays' own type: what step_finish left
    return r


def _wbar_ref(r, blocks=None):
    """Wbar = sum_k diag(2 vbar_k) W B_k + locbar^T U - 2 diag(asum) W; blocks: the reduction index range of the B_k term (all)."""
    W, S = r["W"], r["S"]
    sl = slice(None) if blocks is None else slice(*blocks)
    out = r["locbar"].T @ r["U"] - 2 * r["asum"][:, None] * W
    for k in range(S.shape[0]):
        out += (2 * r["vbar"][k])[:, None] * (W[:, sl] @ (S[k][sl] @ S[k].T))
    return out


def _refs(r):
    W, S, vbar = r["W"], r["S"], r["vbar"]
    return dict(Wbar=_wbar_ref(r), tt=np.stack([((W @ S[k]) ** 2).sum(1) for k in range(S.shape[0])]), loc=r["U"] @ W.T,
                A=np.tril(np.einsum("nk,ni,nj->kij", vbar.T, W, W, optimize=True)), GT=W.T @ r["Wbar"], ubar=r["locbar"] @ W)


def _tile_err(got, ref, rt, ct):
    """max over tiles (rt x ct over the last two axes, leading axes apart) of max |got - ref| / max |ref| inside the tile"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    *lead, R, Cn = ref.shape
    nr, nc = -(-R // rt), -(-Cn // ct)
    pad = [(0, 0)] * len(lead) + [(0, nr * rt - R), (0, nc * ct - Cn)]
    e = np.pad(np.abs(got - ref), pad).reshape(*lead, nr, rt, nc, ct).max(axis=(-3, -1))
    m = np.pad(np.abs(ref), pad).reshape(*lead, nr, rt, nc, ct).max(axis=(-3, -1))
    return float(np.where(m > 0, e / np.where(m > 0, m, 1.0), np.where(e > 0, np.inf, 0.0)).max())


# tiles of each output: Wbar (n, M) and G^T (M, M) in 128 x 128 tiles; tt, loc (K, n) and ubar (K, M) per topic and 128-wide tile; A_k per topic
TILES = dict(Wbar=(TILE, TILE), tt=(1, TILE), loc=(1, TILE), A=(TILE, TILE), GT=(TILE, TILE), ubar=(1, TILE))


def _errors(got, ref):
    return {q: (relerr(got[q], ref[q]), _tile_err(got[q], ref[q], *TILES[q])) for q in TILES}


# id: (K, M, rows, arrays, engine keywords, forms the step must take); n_cap = rows unless "n_cap" is given
CASES = {
    # f16x3 (the default): the k64 W-bar form, its few-row slices (pairs x ceil(Mp / 128) <= 32) and the slab sum
    "f16_k64_K2_nslice4": (2, 256, 4096, "f32", {}, dict(wbar="k64", wbar_nslice=4, a_k="tn_topics", fwd_t="q4", loc="rows", ubar_q4=1)),
    "f16_k64_K8_odd_tiles_nslice4": (8, 256, 3900, "f32", {}, dict(wbar="k64", wbar_nslice=4)),
    "f16_k64_K32_nslice1": (32, 256, 4097, "f32", {}, dict(wbar="k64", wbar_nslice=1, a_k="w2", a_k_kgroups=4, loc="gemm_nt")),
    "f16_k64_K5_Mp128_nslice2": (5, 100, 2000, "f32", {}, dict(wbar="k64", wbar_nslice=2, ubar_q4=2)),
    "f16_k64_K16_minibatch40": (16, 256, 40, "f32", dict(n_cap=5000), dict(wbar="k64", wbar_nslice=4)),
    # f16x3, the other W-bar forms
    "f16_cc_K32_Mp160": (32, 144, 2000, "f32", {}, dict(wbar="split_cc", fwd_t_kg=32)),
    "f16_cc_K33": (33, 256, 1500, "f32", {}, dict(wbar="split_cc", rows="thread")),
    "f16_cc_K64": (64, 256, 1500, "f32", {}, dict(wbar="split_cc", a_k="w2", a_k_kgroups=7)),
    "f16_sp2_K65_Mp224": (65, 200, 1500, "f32", {}, dict(wbar="split<2>")),
    "f16_sp2_K96": (96, 256, 1200, "f32", {}, dict(wbar="split<2>")),
    "f16_sp1_K1": (1, 256, 1500, "f32", {}, dict(wbar="split<1>", fwd_t_kg=1, ubar_q4=1, mm_chain="split8", mm_sbar="direct")),
    "f16_sp1_K97_Mp128": (97, 128, 1500, "f32", {}, dict(wbar="split<1>", fwd_t="q4", fwd_t_kg=51)),
    "f16_sp1_K128_Mp128": (128, 128, 1500, "f32", {}, dict(wbar="split<1>", fwd_t_kg=51, a_k="w2", a_k_kgroups=13)),
    "f16_sp1_K127_Mp160": (127, 160, 1000, "f32", {}, dict(wbar="split<1>", fwd_t_kg=32, ubar_q4=4)),
    "f16_hyper_tn_K128": (128, 128, 1000, "f32", dict(hyper_backward="tn"), dict(wbar="split<1>", hyper="tn", gt="tn_split")),
    # bf16x6
    "bf16_cc_K16": (16, 144, 1500, "f32", dict(mfma_mode="bf16x6"), dict(wbar="split_cc", fwd_t="cc", a_k="tn_split", gt="tn_split")),
    "bf16_sp2_K17": (17, 256, 1500, "f32", dict(mfma_mode="bf16x6"), dict(wbar="split<2>", ubar_q4=4)),
    "bf16_sp2_K64": (64, 200, 1200, "f32", dict(mfma_mode="bf16x6"), dict(wbar="split<2>")),
    "bf16_sp1_K65": (65, 128, 1200, "f32", dict(mfma_mode="bf16x6"), dict(wbar="split<1>", fwd_t_kg=34)),
    "bf16_sp1_K128": (128, 160, 1000, "f32", dict(mfma_mode="bf16x6"), dict(wbar="split<1>", fwd_t_kg=21)),
    # native f32 MFMA, the stored-T W-bar form, fp64 (K > 64: loc on two column tiles)
    "f32_K64": (64, 128, 1200, "f32", dict(mfma_mode="f32"), dict(wbar="gemm_nt", a_k="gemm_tn", fwd_t="gemm_nt", gt="gemm_tn")),
    "f32_K65": (65, 160, 1000, "f32", dict(mfma_mode="f32"), dict(wbar="gemm_nt")),
    "f32_K128": (128, 128, 1000, "f32", dict(mfma_mode="f32"), dict(wbar="gemm_nt", loc="gemm_nt")),
    "store_t_K33": (33, 128, 1000, "f32", dict(store_t=True), dict(wbar="gemm_nt_t")),
    "store_t_K128": (128, 128, 1000, "f32", dict(store_t=True), dict(wbar="gemm_nt_t")),
    "f64_K64": (64, 128, 1000, "f64", {}, dict(wbar="gemm_nt", loc="gemm_nt")),
    "f64_K65": (65, 128, 1000, "f64", {}, dict(loc="gemm_nt_wide")),
    "f64_K128": (128, 160, 800, "f64", {}, dict(loc="gemm_nt_wide", ubar_q4=4)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_stage_forms_against_fp64_products_of_the_engine_inputs(case):
    K, M, n, arrays, kw, forms = CASES[case]
    kw = dict(kw)
    n_cap = kw.pop("n_cap", n)
    d = _inputs(K, M, n)
    eng = _engine(d, n_cap, torch.float64 if arrays == "f64" else torch.float32, **kw)
    got = _step(eng, d)
    seen = eng.last_forms()
    errs = _errors(got, _refs(got))
    kind = "f64" if arrays == "f64" else ("f32" if eng.mfma_mode == "f32" else "split")
    print(case, seen)
    for q, (g, t) in errs.items():
        print("   %-5s global %.2e (bound %.0e)  per tile %.2e (bound %.0e)" % (q, g, GLOBAL[kind][q], t, TILE_TOL))
    assert {k: seen.get(k) for k in forms} == forms, (case, seen)
    # the same step again on the same engine: bit-identical (fixed accumulation order)
    again = _step(eng, d)
    for q in ("Wbar", "tt", "A", "GT", "grads"):
        assert np.array_equal(got[q], again[q]), (case, q, float(np.abs(got[q] - again[q]).max()))
    assert np.isfinite(got["grads"]).all() and np.isfinite(again["grads"]).all(), case
    for q, (g, t) in errs.items():
        assert g < GLOBAL[kind][q] and t < TILE_TOL, (case, q, g, t)


# ---- end to end at large K: every gradient block against autograd of the fp64 oracle ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("K", [33, 65, 97, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_all_gradient_blocks_at_large_topic_counts(K, dtype):
    from tests.test_gpu_round3 import BLOCKS, LOSS_TOL_FP64, REGIMES, _all_block_errors, _assert_fp32, _fp32_valued
    m, eps = make_oracle(kind="rbf", W=50, H=40, V=12, K=K, n_points=(10, 10), dtype=torch.float64, jitter=1e-6, lengthscale=0.15,
                         **REGIMES["trained"])
    if dtype == torch.float32:
        _fp32_valued(m)
    lvl, errs, eng = _all_block_errors(m, eps, dtype)
    print("K", K, dtype, "level", lvl, eng.last_forms(), {k: f"{v:.2e}" for k, v in errs.items()})
    if dtype == torch.float32:
        assert eng.mfma_mode == "f16x3"
        _assert_fp32(errs, "trained")
    else:
        assert errs["loss"] < LOSS_TOL_FP64
        for name in BLOCKS:
            assert errs[name] < 1e-7, (name, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_predictive_modes_at_128_topics(dtype):
    """gdrf_predict modes 0-4 past the K <= 32 matrix-core predictive form (the topic-chunked row kernel)."""
    from tests.test_gpu_round3 import test_predictive_modes_and_loc_var_against_the_oracle as run
    run(dict(kind="rbf", W=30, H=20, V=11, K=128, n_points=(6, 5)), dtype)


# ---- CPU: the measures above see each simulated fault ---------------------------------------------------------------------------------

def _synthetic(n=4097, M=256, K=8, seed=5):
    """Operands shaped like the engine's, with the same loud topic K-1 and loud last row tile."""
    rng = np.random.default_rng(seed)
    last = (n - 1) // TILE * TILE
    vbar, locbar = 0.1 * rng.standard_normal((K, n)), 0.1 * rng.standard_normal((K, n))
    vbar[K - 1] *= 4
    vbar[:, last:] *= 10
    locbar[:, last:] *= 10
    S = 0.1 * np.tril(rng.standard_normal((K, M, M)))
    S[K - 1] *= 3
    r = dict(W=0.3 * rng.standard_normal((n, M)), S=S, vbar=vbar, locbar=locbar, asum=rng.random(n), U=0.3 * rng.standard_normal((K, M)))
    r["Wbar"] = _wbar_ref(r)
    return r, last


def test_tile_measures_see_a_doubled_topic_a_lost_row_tile_and_a_missing_slice():
    r, last = _synthetic()
    ref = _refs(r)
    K = r["S"].shape[0]
    bound = GLOBAL["split"]
    faults = {}
    w = ref["Wbar"] + (2 * r["vbar"][K - 1])[:, None] * (r["W"] @ (r["S"][K - 1] @ r["S"][K - 1].T))      # topic K-1 counted twice
    faults["Wbar: topic K-1 doubled"] = (w, ref["Wbar"], "Wbar")
    t = ref["tt"].copy()
    t[K - 1] *= 2
    faults["tt: topic K-1 doubled"] = (t, ref["tt"], "tt")
    a = ref["A"].copy()
    a[K - 1] *= 2
    faults["A_k: topic K-1 doubled"] = (a, ref["A"], "A")
    w = ref["Wbar"].copy()
    w[last:] = 0
    faults["Wbar: last row tile lost"] = (w, ref["Wbar"], "Wbar")
    t = ref["tt"].copy()
    t[:, last:] = 0
    faults["tt: last row tile lost"] = (t, ref["tt"], "tt")
    # the k64 form's slice 1 of 4 (reduction indices 64 .. 127 at Mp = 256) missing from the slab sum
    faults["Wbar: one of 4 slices missing"] = (ref["Wbar"] - (_wbar_ref(r, (64, 128)) - _wbar_ref(r, (0, 0))), ref["Wbar"], "Wbar")
    for name, (got, want, q) in faults.items():
        g, tl = relerr(got, want), _tile_err(got, want, *TILES[q])
        print("%-32s global %.2e  per tile %.2e" % (name, g, tl))
        assert g > 100 * bound[q] and tl > 100 * TILE_TOL, (name, g, tl)
    # and an exact result passes both
    for q in TILES:
        assert relerr(ref[q], ref[q]) == 0 and _tile_err(ref[q], ref[q], *TILES[q]) == 0
