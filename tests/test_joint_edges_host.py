"""CPU tests of tests/_joint_ref.py: the shapes of tests/test_gpu_joint_edges.py cross the loop bounds their comments name, the all-fp32
bounds stay under the ceiling, and the measures see the faults those shapes exist for.

The faults, each simulated in the float64 restatement at the case's own inputs and held against 100 times the case's bound (1e-7 and 1e-4
in the float64 and float32 contexts, the computed one in the all-fp32 context):
  - a loop over Mp that skips one 32-column block of W: every block of every shape in turn, on C_k, R, the samples, the first gains and
    the conditional variances after the picks;
  - a chol_kernel that leaves out its second 256-column chunk, its second strip group, or stage (c)'s second round: on the samples.
"""
import os
import re

import numpy as np
import pytest

from tests import _joint_ref as R

if not R.P.HAS_LONGDOUBLE:
    pytest.skip("np.longdouble has no more precision than float64 here: the exact restatement needs eps < 1e-18", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOUD = 100.0
FLOOR = R.FLOOR32
ENGINE = [(name, e["id"], ctx) for name in ("cov", "select", "sample") for e in R._list(name).values() for ctx in e["ctxs"]]
MODEL = [(K, S, n, ctx) for ctx in R.CTXS for (K, S, n) in
         [(1, 2, n) for n in R.SAMPLE_N[ctx]] + [(K, S, R.SAMPLE_SK_N) for K, S in R.SAMPLE_SK]]


def csrc(name):
    return open(os.path.join(ROOT, "gdrf_amd", "csrc", name)).read()


def test_the_restated_tile_sizes_are_the_headers():
    define = lambda src, name: int(re.search(r"#define %s (\d+)\b" % name, src).group(1))
    common, mm, cov, sel = csrc("common.h"), csrc("kernels_mm.h"), csrc("predict_cov.h"), csrc("select_batch.h")
    assert define(common, "GDRF_MPAD") == R.MPAD
    assert define(mm, "CHOL_PC") == R.CHOL_PC
    assert define(cov, "GDRF_JT") == R.JT
    assert define(sel, "GDRF_SEL_COLS") == R.SEL_COLS and define(sel, "GDRF_SEL_ROWS") == R.JT
    assert "constexpr int NS = sizeof(T) == 4 ? %d : %d;" % (R.CHOL_NS[4], R.CHOL_NS[8]) in mm
    assert "for (int i0 = c0 + 32; i0 < M; i0 += %d)" % R.CHOL_ROUND in mm
    assert "for (int q = gl * VE; q < Mp; q += 16 * VE)" in sel
    # Vec16<T>::N is 16 bytes' worth of T
    assert re.search(r"struct Vec16<float>\s*\{[^}]*N = %d" % R.VEC[4], common + mm) and re.search(r"struct Vec16<double>\s*\{[^}]*N = %d" % R.VEC[8], common + mm)


@pytest.mark.parametrize("name", ["cov", "select", "sample"])
def test_each_shape_crosses_what_its_comment_names(name):
    for e in R._list(name).values():
        assert e["expect"], e["id"]
        for ts, want in e["expect"].items():
            assert any(R.TS[c] == ts for c in e["ctxs"]), (e["id"], ts)
            got = R.crossings(ts, M=e["M"], K=e["K"], SK=e.get("S", 0) * e["K"])
            assert {k: got[k] for k in want} == want, (e["id"], ts, got)
        assert int(np.prod(e["grid"])) >= e["M"] and len(e["grid"]) == e["D"]


def test_the_sample_shapes_cross_the_cholesky_and_tile_edges():
    for n, per_ts in R.SAMPLE_N_EXPECT.items():
        for ts, want in per_ts.items():
            got = R.crossings(ts, n=n)
            assert {k: got[k] for k in want} == want, (n, ts, got)
    for ctx in R.CTXS:
        assert set(R.SAMPLE_N[ctx]) <= set(R.SAMPLE_N_EXPECT)
    # what the shapes are for: the smallest n that reaches each loop's second round, per element size
    first = lambda key, ts: next(n for n in range(33, 4096) if R.crossings(ts, n=n)[key] >= 2)
    assert first("chol_chunks", 8) == 289 and first("chol_strip_groups", 8) == 545 and first("chol_strip_groups", 4) == 1057
    assert first("chol_rounds", 8) == 1057
    assert R.crossings(8, n=257)["chol_chunks"] == 1                     # n = 257 stays within the first chunk
    assert {K * S: R.crossings(8, SK=K * S)["sample_tiles"] for K, S in R.SAMPLE_SK} == R.SAMPLE_SK_EXPECT
    assert R.crossings(8, M=R.PHILOX_CASE["M"], SK=R.PHILOX_CASE["S"] * R.PHILOX_CASE["K"])["sample_tiles"] == 3
    # the all-fp32 stride of 64 on the existing Mp = 32 and on Mp = 96
    assert R.crossings(4, M=12)["dot_rounds"] == (0, 1) and R.crossings(4, M=65)["dot_rounds"] == (1, 2)


def bounds_of(maker, key, ctx):
    """{quantity: bound} of a case in a context type"""
    if ctx == "pure":
        b = R.pure_reference(maker, *key)[2]
        assert max(b.values()) <= R.CEILING, (key, b)
        return b
    return dict.fromkeys(("C", "R", "f", "gain0", "gain_last", "dvar"), R.TOL[ctx])


@pytest.mark.parametrize("name,id,ctx", [c for c in ENGINE if c[2] == "pure"])
def test_the_all_fp32_bounds_stay_under_the_ceiling(name, id, ctx):
    for n in R._list(name)[id]["ns"]:
        b = R.pure_reference(R.engine_inputs, name, id, ctx, n)[2]
        print(name, id, n, {k: "%.2e" % v for k, v in b.items()})
        assert FLOOR <= min(b.values()) and max(b.values()) <= R.CEILING, (n, b)


@pytest.mark.parametrize("K,S,n,ctx", [c for c in MODEL if c[3] == "pure"])
def test_the_all_fp32_sample_bounds_stay_under_the_ceiling(K, S, n, ctx):
    inp, exact, b = R.pure_reference(R.model_inputs, K, S, n, ctx)
    print(K, S, n, {k: "%.2e" % v for k, v in b.items()})
    assert not exact["chol_failed"]
    assert FLOOR <= min(b.values()) and max(b.values()) <= R.CEILING, b


@pytest.mark.parametrize("name,id,ctx", ENGINE)
def test_a_skipped_block_of_W_is_seen(name, id, ctx):
    """every 32-column block of W, M = 33's single real column included, on every checked quantity"""
    e = R._list(name)[id]
    n = 65
    inp, kw = R.engine_inputs(name, id, ctx, n)
    if inp["xi"] is None:                                               # every shape is checked on the samples as well
        case = R.make_case(e, ctx)
        xi, zeta = R.normals(2, e["K"], e["M"], inp["X"].shape[0], case.dtype)
        inp = dict(inp, xi=np.asarray(xi), zeta=np.asarray(zeta), jrow=case.jitter)
    bound = bounds_of(R.engine_inputs, (name, id, ctx, n), ctx)
    bound.setdefault("f", max(bound.values()))
    good = R.restate(inp, np.float64, **kw)
    picks = R.greedy_picks(good, R.COUNT, e["given"])                     # the picks of the unfaulted rule, held fixed
    good = R.restate(inp, np.float64, picks=picks, **kw)
    for b in range(R.crossings(8, M=e["M"])["Mp"] // 32):
        moved = R.measures(R.restate(inp, np.float64, zero_block=b, picks=picks, **kw), good)
        for q in ("C", "R", "f", "gain0", "dvar"):
            print(name, id, ctx, "block", b, q, "moved %.2e, bound %.2e" % (moved[q], bound[q]))
            assert moved[q] > LOUD * bound[q], (b, q, moved[q], bound[q])


@pytest.mark.parametrize("K,S,n,ctx", MODEL)
def test_a_defective_cholesky_is_seen(K, S, n, ctx):
    """the samples move by more than 100 bounds when the factorisation leaves out what the shape exists to reach (or a pivot fails: the
    kernel's flag, which the engine answers with another jitter level)"""
    ts = R.TS[ctx]
    inp, kw = R.model_inputs(K, S, n, ctx)
    bound = bounds_of(R.model_inputs, (K, S, n, ctx), ctx)["f"]
    good = R.restate(inp, np.float64, ts=ts)
    assert not good["chol_failed"]
    c = R.crossings(ts, n=n)
    drops = [d for d, key in (("chunk", "chol_chunks"), ("strips", "chol_strip_groups"), ("round", "chol_rounds")) if c[key] >= 2]
    if n in R.SAMPLE_N_EXPECT and n != 288:
        assert drops, (n, ts)
    for d in drops:
        with np.errstate(all="ignore"):                                  # a defective factor may overflow: measures() then says inf
            bad = R.restate(inp, np.float64, drop=d, ts=ts)
        moved = R.measures(bad, good)["f"]
        print(K, S, n, ctx, d, "moved %.2e, bound %.2e, pivot failed: %s" % (moved, bound, bad["chol_failed"]))
        assert bad["chol_failed"] or moved > LOUD * bound, (d, moved, bound)
    # the single 32-column block of W at M = 20
    moved = R.measures(R.restate(inp, np.float64, zero_block=0, ts=ts), good)["f"]
    assert moved > LOUD * bound, (moved, bound)


def test_the_block_cholesky_is_a_cholesky():
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 100, 300):
        B = rng.standard_normal((n, n))
        A = B @ B.T + n * np.eye(n)
        L, bad = R.block_cholesky(A)
        assert not bad and np.abs(L - np.linalg.cholesky(A)).max() <= 1e-12 * np.abs(L).max()
    L, bad = R.block_cholesky(-np.eye(3))
    assert bad and np.isfinite(L).all()
