"""CPU tests of tests/_side_ref.py: the tables of tests/test_gpu_side_edges.py test what they claim, shown from the reference alone.

  - every case's oracle is finite at its own jitter level, and the row reference agrees with it (d / d u_loc from the row adjoints);
  - in every clamp case the clamp is active at the chosen word on every row, the word carries real weight, and a normaliser taken over ALL
    counts (a `cn` that forgot the clamp) moves locbar and d / d u_loc by more than 100 x the bound the GPU test applies in fp64 (the float32
    clamp case is there for the element type's clamp threshold: a count of 3 moves d / d u_loc by 7e-2 there, 3.7 x its 2e-2 bound);
  - the link path's cancellation floor is under 5 % of the bound wherever K > 1;
  - the sigmoid link does not sum to one, so `cn` and `cpart` matter; the two-point objective differs from the single-point one;
  - the shapes cross the edges their names state, recomputed from the constants of the headers, which are tied to their source lines."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _side_ref as R
from tests._util import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64_G, TOL64_ROWS_ADJ = 1e-7, 1e-8 * 10          # the GPU test's fp64 bounds: per gradient block; vbar / locbar (10 x TOL["w"])
TOL32_G = 2e-2                                     # float32: TOL[float32]["g"]
LOUD = 100.0
_cache = {}


def built(cid):
    """(case, oracle, eps, xs_world, loss, grads) at the oracle's own jitter level, once per case"""
    if cid not in _cache:
        c = R.CASES[cid]
        m, eps, xs_w = R.build(c)
        loss, grads = R.oracle_loss_and_grads(m, c, eps)
        _cache[cid] = (c, m, eps, xs_w, loss, grads, m.last_jitter_level)
    return _cache[cid]


def csrc(name):
    return open(os.path.join(ROOT, "gdrf_amd", "csrc", name)).read()


ALL = list(R.CASES)
CLAMP = [cid for cid, c in R.CASES.items() if c["clamp_word"] is not None]
SIGMOID = [cid for cid, c in R.CASES.items() if c["link"] == "sigmoid"]
TWO = [c["id"] for c in R.TWO_CASES]


def test_the_restated_constants_are_the_sources():
    vs, api, forms = csrc("rows_vstream.h"), csrc("api.hip"), csrc("forms.h")
    assert "static constexpr int RB = %d;" % R.RB in vs
    assert "static constexpr int VT = sizeof(T) == 8 ? %d : %d;" % (R.VT[8], R.VT[4]) in vs
    assert "rc = c->K <= %d ? go(rows_vstream_kernel<T, MODE, 8>) : go(rows_vstream_kernel<T, MODE, 32>);" % R.KJ_SPLIT in api
    assert "return K <= 8 ? f(LaneForm<8, 1>()) : K <= 32 ? f(LaneForm<16, 2>()) : f(LaneForm<16, 8>());" in api
    assert [R.sparse_form(K) for K in (8, 9, 32, 33, 128)] == [(8, 1), (16, 2), (16, 2), (16, 8), (16, 8)]
    assert "c->vs_gcap = std::min<int64_t>({(int64_t)%d, std::max<int64_t>(16, (int64_t)((size_t)256 << 20) / (int64_t)kv), (c->ncap + 63) / 64});" % R.GRID_MAX in api
    assert R.GCAP_BYTES == 256 << 20
    assert "std::min<int64_t>((n + 63) / 64, c->csr_crow && counts ? %d : c->vs_gcap)" % R.GRID_MAX in api
    assert "constexpr int F_TILE = %d;" % R.F_TILE in forms
    assert "return (f.Mp %% 64) == 0 && f.K >= 2 && f.K <= 16 && pairs * f.nt() > %d;" % R.W1_PAIRS in forms
    assert "if (pairs * nct <= %d && nkb >= 2) p.nslice = std::min(nkb, 8);" % R.W1_PAIRS in forms
    assert re.search(r"int64_t ldk\(\) const \{ return \(n_cap \+ 3\) / 4 \* 4; \}", forms)


def test_the_tables_hold_the_cases_the_sweep_names():
    ids = set(R.CASES)
    for regime in ("fp64", "fp32"):
        for K, V in R.LINK_EDGES:
            assert {f"link-sigmoid-K{K}-V{V}-{regime}", f"link-tempered_softmax-K{K}-V{V}-{regime}"} <= ids
        for K, V in R.TWO_EDGES:
            assert f"two-K{K}-V{V}-{regime}" in ids
    assert R.LINK_EDGES == [(1, 1), (1, 2), (8, 31), (9, 32), (32, 33), (33, 63), (33, 64), (33, 65), (128, 33), (128, 65)]
    assert R.TWO_EDGES == [(1, 2), (9, 32), (32, 64), (33, 65), (128, 33)]
    assert [(R.CASES[c]["K"], R.CASES[c]["V"]) for c in CLAMP if c.endswith("fp64") and "csr" not in c] == R.LINK_CLAMP
    csr = [(c["K"], c["density"]) for c in R.LINK_CASES if c["route"] == "csr" and c["regime"] == "fp64" and c["clamp_word"] is None and c["V"] == 50]
    assert csr == [(K, d) for K in (8, 9, 32, 33, 128) for d in (0.05, 1.0)]
    kinds = {c["kind"] for c in R.TWO_CASES}
    assert kinds == {"rbf", "matern52", "matern32", "exponential", "rationalquadratic"}
    assert {c["mfma_mode"] for c in R.TWO_CASES if c["regime"] == "fp32"} == {"f16x3", "bf16x6", "f32"}
    for c in R.CASES.values():
        assert c["zero_rows"] == 3 and (c["link"] is None) == (c["path"] == "two")


@pytest.mark.parametrize("cid", ALL)
def test_derived_counts(cid):
    c = R.CASES[cid]
    d = R.derived(c)
    K, V, esz = c["K"], c["V"], 8 if c["regime"] == "fp64" else 4
    assert d["KJ"] * 4 >= K and (d["KJ"] == 8) == (K <= 32)
    assert d["LG"] * d["csr_KJ"] >= K
    assert d["ldk"] % 4 == 0 and d["ldk"] >= d["n"]
    if cid == "link-capped-grid-K128-V4100":
        assert (d["row_blocks"], d["grid"], d["blocks_per_wg"]) == (64, 63, 2)        # one workgroup carries two row blocks
    elif cid == "link-csr-two-blocks-per-workgroup":
        assert d["n"] == 1024 * 64 + 37 and d["grid"] == 1024 and d["row_blocks"] == 1025 and d["blocks_per_wg"] == 2
    else:
        assert d["blocks_per_wg"] == 1
    if c["lattice"] == (37, 9):
        assert (d["n"], d["row_blocks"], d["ragged"]) == (333, 6, 13)                # five full 64-row blocks and a ragged one of 13
        assert d["Mp"] > int(np.prod(c["n_points"])) or c["n_points"] != (4, 3)      # M = 12 is padded to Mp = 32
    if c["n_cap"]:
        assert c["n_cap"] == 401 and d["ldk"] == 404 and d["ldk"] != d["n"]
    if c["forms"]:
        assert d["w1"] == (c["forms"]["wbar"] == "w1") and d["nslice"] == c["forms"]["wbar_nslice"], d
        if d["w1"]:
            assert d["pairs"] == 34 and d["pairs"] * d["nt"] > R.W1_PAIRS and d["n"] == 8633
    # the V edges: on the dense route a tile of VT words, both sides of one and of two tiles
    assert d["vt_tiles"] == -(-V // R.VT[esz])


def test_the_edge_lists_cross_every_edge():
    tiles = {esz: {(-(-V // vt), V % vt == 0) for _, V in R.LINK_EDGES} for esz, vt in R.VT.items()}
    assert {(1, False), (1, True), (2, False)} <= tiles[8] and {(1, False), (1, True), (2, False)} <= tiles[4]      # below, at and past one tile
    assert {K for K, _ in R.LINK_EDGES} >= {1, 8, 9, 32, 33, 128} and {K for K, _ in R.TWO_EDGES} >= {1, 9, 32, 33, 128}


@pytest.mark.parametrize("cid", ALL)
def test_oracle_is_finite_and_the_row_reference_agrees_with_it(cid):
    c, m, eps, _, loss, grads, level = built(cid)
    assert np.isfinite(loss) and set(grads) == set(m.params)
    for name, g in grads.items():
        assert torch.isfinite(g).all(), name
    if c["path"] == "two":      # the two-point objective IS another one: a step that ignored xs_guide would be far off
        e1 = eps[-1] if eps.dim() == 3 else eps
        m.force_jitter_level = level
        two = float(m.loss(e1).detach())
        m.guide_rescale = False
        try:
            single = float(m.loss(e1).detach())
        finally:
            m.guide_rescale = True
        assert abs(single - two) > 1e-3 * abs(two), (single, two)
    if c["renyi"] is not None:
        return                  # the particle weights are not the rows' business
    # d loss / d u_loc from the row adjoints (mean over the particles) against autograd through the whole oracle
    es = eps if eps.dim() == 3 else eps[None]
    g_rows = sum(R.u_loc_grad_from_rows(m, R.row_reference(m, e, level)) for e in es) / len(es)
    # (+ ABS_FLOOR: at V = 1 the likelihood has no gradient and the two Normal sites cancel, so autograd's own answer is round-off around 0)
    assert float((g_rows - grads["u_loc"]).abs().max()) <= 1e-10 * float(grads["u_loc"].abs().max()) + R.ABS_FLOOR


@pytest.mark.parametrize("cid", CLAMP)
def test_clamp_cases_have_the_clamp_active_and_would_catch_a_normaliser_over_all_counts(cid):
    c, m, eps, _, loss, grads, level = built(cid)
    vc, fe = c["clamp_word"], np.finfo(np.float64).eps
    ref = R.row_reference(m, eps, level)
    has = m.ws.sum(1) > 0
    assert bool((ref["p_hat"][:, vc] < fe).all())                            # in EVERY row
    share = m.ws[:, vc].double() / m.ws.sum(1).clamp(min=1).double()
    assert float((share >= 0.01).double().mean()) >= 0.5                     # the clamped word carries weight
    assert bool((m.ws[has, vc] == 3).all())
    # the clamped column of phi_unc sees the Dirichlet prior alone
    assert relerr(grads["phi_unc"][:, vc].numpy(), R.dirichlet_grad(m)[:, vc].numpy()) < 1e-12
    if (c["K"], c["V"]) == (1, 2):
        # the other word sits at the upper clamp 1 - eps: the likelihood's whole gradient vanishes
        assert bool((ref["p_hat"][:, 1 - vc] >= 1 - fe).all())
        assert float(ref["locbar"].abs().max()) == 0.0 and float(grads["u_loc"].abs().max()) <= R.ABS_FLOOR
    wrong = R.row_reference(m, eps, level, normaliser="all")
    if c["regime"] == "fp32":
        # the float32 case is there for the clamp threshold of the element type and the loss shift that goes with it.  A count of 3 on the
        # clamped word moves d / d u_loc by 7e-2 under the fault: visible, but not 100 x float32's 2e-2 - the fp64 cases carry that proof
        assert abs(R.eps32_loss_shift(m, c)) > 1e-2 * abs(loss)
        assert relerr(R.u_loc_grad_from_rows(m, wrong).numpy(), R.u_loc_grad_from_rows(m, ref).numpy()) > TOL32_G
        return
    tol_g, tol_adj = TOL64_G, TOL64_ROWS_ADJ
    d_adj = relerr(wrong["locbar"].numpy(), ref["locbar"].numpy())
    d_u = relerr(R.u_loc_grad_from_rows(m, wrong).numpy(), R.u_loc_grad_from_rows(m, ref).numpy())
    print(cid, "normaliser over all counts: locbar off by %.3g, d/d u_loc by %.3g" % (d_adj, d_u))
    assert d_adj > LOUD * tol_adj and d_u > LOUD * tol_g, (d_adj, d_u)


@pytest.mark.parametrize("cid", [c["id"] for c in R.LINK_CASES if c["K"] > 1])
def test_the_cancellation_floor_loosens_no_case_with_more_than_one_topic(cid):
    c, m, eps, _, _, _, level = built(cid)
    ref = R.row_reference(m, eps[-1] if eps.dim() == 3 else eps, level)
    fp32 = c["regime"] == "fp32"
    floor = R.link_cancellation_floor(m, ref, c["V"], float(np.finfo(np.float32 if fp32 else np.float64).eps))
    bound = (2e-3 if fp32 else 1e-8) * 10 * float(ref["locbar"].abs().max())          # what the GPU test allows vbar and locbar
    assert float(floor.max()) < 0.05 * bound, (float(floor.max()), bound)


@pytest.mark.parametrize("cid", SIGMOID)
def test_sigmoid_link_does_not_sum_to_one(cid):
    c, m, eps, _, _, _, level = built(cid)
    ref = R.row_reference(m, eps[-1] if eps.dim() == 3 else eps, level)
    assert float((ref["theta"].sum(0) - 1.0).abs().min()) > 1e-2


@pytest.mark.parametrize("cid", ALL)
def test_data_are_loud(cid):
    c, m, eps, _, _, _, _ = built(cid)
    ws, K, V = m.ws.numpy().astype(np.int64), c["K"], c["V"]
    tot = ws.sum(1)
    assert int((tot == 0).sum()) >= 3 and (c["density"] < 1.0 or int((tot == 0).sum()) == 3) and tot[-1] > 20 * np.median(tot[tot > 0])
    if V > 1 and c["clamp_word"] != V - 1:         # (at V = 2 the clamped word, with its count of 3, IS the last one)
        assert ws[:-1].sum(0).argmax() == V - 1
    if K > 1:
        u = m.params["u_loc"].detach()
        assert int(u.abs().amax(1).argmax()) == K - 1
    if c["regime"] == "fp32":
        for name, p in m.params.items():
            assert torch.equal(p.detach(), p.detach().float().double()), name
        assert torch.equal(eps, eps.float().double()) and torch.equal(m.Z, m.Z.float().double())
