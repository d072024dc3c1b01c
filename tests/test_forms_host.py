"""CPU: the rules that pick a kernel form per stage (gdrf_amd/csrc/forms.h), checked without a GPU through the stand-alone table program
tests/host/forms_table.cpp, built once per session with the host compiler.

1. Every case of the five GPU form tests (their own tables: SHAPES of test_gpu_wbar_w1 and test_gpu_fwd_t_w1, CASES of test_gpu_topic_forms,
   GROUPS of _predict_ref, A_CASES and B_CASES of test_gpu_finish_k1) still reaches the form it asserts on the GPU, so a change of a
   threshold shows here and not only on a GPU.
2. A sweep with both sides of every threshold against tests/_forms_ref.py, an independent Python statement of the rules: every slot and the
   split counts of A_k, G^T and the hyper-TN form.
3. The highest code of each named slot is the number of names Engine.FORM_NAMES has for it.
4. The M x M products of step_finish (mm_plan; slots mm_chain and mm_sbar): the table against the restatement, the edges of the split-K gate,
   and the invariant that Sbar_k = 2 A_k S_k, which the whitened form runs on the side stream beside the Cholesky-backward chain, never
   goes through the slab buffer the chain's products go through - with the old rule kept as a simulated fault that the invariant catches."""
import itertools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from gdrf_amd.engine import Engine
from tests import _forms_ref as FR
from tests import _predict_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = Engine.FORM_SLOTS


@pytest.fixture(scope="session")
def table(tmp_path_factory):
    """Path of the built table program; no compiler is a failure, not a skip."""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm if os.path.exists(rocm) else None)
    assert cxx, "no host C++ compiler: neither c++ on PATH nor ROCm's clang++"
    exe = str(tmp_path_factory.mktemp("forms") / "forms_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "forms_table.cpp")], check=True)
    return exe


def _run(table, shapes):
    """The program's rows for the shapes: a dict per shape with the slots' numbers and the split counts."""
    out = subprocess.run([table], input="".join(FR.line(s) + "\n" for s in shapes), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(shapes), (len(out), len(shapes))
    return [dict(zip(SLOTS + FR.EXTRA, map(int, row.split()))) for row in out]


def _named(row):
    """The row as Engine.last_forms() reports it: names for the form slots, counts for the others, stages that did not run left out."""
    return {k: (Engine.FORM_NAMES[k][row[k] - 1] if k in Engine.FORM_NAMES else row[k]) for k in SLOTS if row[k]}


def _gpu_cases():
    """(id, shape, forms the GPU test asserts, slots it asserts to be unset)"""
    from tests import test_gpu_finish_k1, test_gpu_fwd_t_w1, test_gpu_topic_forms, test_gpu_wbar_w1
    cases = []
    fk = test_gpu_finish_k1                            # engine_from_oracle of make_oracle(W=25, H=16, V=12): n = 400, M = Mp
    for Mp, K, arrays, whiten in ([(Mp, K, a, w) for Mp, K in fk.A_CASES for a in ("f32", "f64") for w in (True, False)]
                                  + [(Mp, 1, a, w) for Mp, a, w in fk.B_CASES]):
        s = FR.resolve(400, Mp, K, 12, dtype="f64" if arrays == "f64" else "f32", pure_fp32=arrays == "pure", whiten=whiten)
        cases.append((f"finish_k1:Mp{Mp}:K{K}:{arrays}:{whiten}", s, fk._want_forms(Mp, K, arrays, whiten), ()))
    for mod, want in ((test_gpu_wbar_w1, lambda K: dict(wbar="w1", wbar_nslice=1)),
                      (test_gpu_fwd_t_w1, lambda K: dict(fwd_t="w1", fwd_t_kg=4 if K >= 4 else 2 * min(2, (K + 1) // 2)))):
        for name, kw in mod.SHAPES.items():         # make_oracle(V=12, **kw) and engine_from_oracle(m, mfma_mode="f16x3", store_t=False, n_cap=n_cap)
            s = FR.resolve(kw["W"] * kw["H"], int(np.prod(kw["n_points"])), kw["K"], 12, n_cap=kw.get("n_cap"), mfma_mode="f16x3", store_t=False,
                           kind=kw.get("kind", "rbf"))
            cases.append((f"{mod.__name__}:{name}", s, want(kw["K"]), ()))
    for name, (K, M, n, arrays, kw, forms) in test_gpu_topic_forms.CASES.items():       # its _engine: V = 12, D = 2, matern52
        cases.append((f"topic_forms:{name}", FR.resolve(n, M, K, 12, dtype=arrays, kind="matern52", **kw), forms, ()))
    for g in PR.GROUPS:                                # test_gpu_predict_forms._engine: n_cap or 64, default arithmetic
        for n, mode in itertools.product(g["ns"], g["modes"]):
            s = FR.resolve(n, g["M"], g["K"], g["V"], g["D"], n_cap=g["n_cap"] or 64, dtype="f64" if g["ctx"] == "f64" else "f32",
                           pure_fp32=g["ctx"] == "pure", rows_form="streamed" if g["streamed"] else "auto", csr=g["csr"], ard=g["ard"],
                           kind=g["kind"], predict_mode=mode)
            if mode == 4:
                cases.append((f"predict:{g['id']}:n{n}:mode4", s, {}, ("predict", "predict_nb")))
            else:
                want = dict(predict=Engine.FORM_NAMES["predict"][g["form"][0] - 1])
                cases.append((f"predict:{g['id']}:n{n}:mode{mode}", s, dict(want, predict_nb=g["form"][1]) if g["form"][1] else want,
                              () if g["form"][1] else ("predict_nb",)))
    return cases


def test_every_gpu_form_case_still_reaches_the_form_it_asserts(table):
    cases = _gpu_cases()
    assert len(cases) > 200
    rows = _run(table, [c[1] for c in cases])
    bad = []
    for (cid, s, want, unset), row in zip(cases, rows):
        seen = _named(row)
        if {k: seen.get(k) for k in want} != want or any(k in seen for k in unset):
            bad.append((cid, want, unset, seen))
    assert not bad, bad


ARITH = {  # arrays / arithmetic -> (esz, ssz, split, stored_t)
    "f16x3": (4, 8, 2, 0), "bf16x6": (4, 8, 1, 0), "f32": (4, 8, 0, 0), "all-fp32": (4, 4, 1, 0), "f64": (8, 8, 0, 0), "stored-T": (4, 8, 0, 1)}
KS = list(range(1, 18)) + [31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 98, 127, 128]
MPS = list(range(32, 641, 32)) + [1024]
NS = [40, 1500, 2000, 4096, 4097, 5000, 100_000, 1_000_000]
VS = [12, 32, 33, 64, 65, 300]


def _sweep():
    """Two crossings, the fields that a crossing leaves out drawn per shape: K x Mp x n x arithmetic (the stages that read K, Mp and n) and
    K x V x row form x predict mode x arithmetic (the row terms and the predictive routes); then the edges that need sizes of their own."""
    rng = random.Random(0)
    shapes = []

    def shape(K, Mp, n, arith, V, rows_form, mode):
        esz, ssz, split, stored_t = ARITH[arith]
        return dict(n=n, n_cap=n * rng.choice((1, 2)), M=Mp - rng.choice((0, 0, 5, 31)), K=K, V=V, D=rng.choice((1, 2, 3, 4)), esz=esz, ssz=ssz,
                    split=split, stored_t=stored_t, rows_form=rows_form, csr=int(rng.random() < 0.1), hyper_tn=rng.choice((0, 1)),
                    learn_z=int(rng.random() < 0.1), ard=int(rng.random() < 0.1), per=int(rng.random() < 0.1), kind=rng.choice(range(5)),
                    predict_mode=mode, unwhitened=(K + Mp // 32 + len(shapes)) % 3 == 0)      # no draw: the shapes of the sweep stay the ones they were

    for K, Mp, n in itertools.product(KS, MPS, NS):          # the split arithmetics, whose forms depend on all three, and one of the others
        for arith in ("f16x3", "bf16x6", rng.choice(("f32", "all-fp32", "f64", "stored-T"))):
            shapes.append(shape(K, Mp, n, arith, rng.choice(VS), rng.choice((0, 1)), rng.choice(range(5))))
    for K, V, rows_form, mode, arith in itertools.product(KS, VS, (0, 1), range(5), ARITH):
        shapes.append(shape(K, rng.choice(MPS), rng.choice(NS), arith, V, rows_form, mode))
    # rows whose 32-bit byte offsets the matrix-core row form cannot hold, beside ones it can
    for n, arith in itertools.product((30_000_000, 40_000_000), ("f32", "f64")):
        shapes.append(shape(32, 64, n, arith, 12, 0, 0))
    # the predictive routes of K <= 32 past the matrix-core form's 64 KiB: vocabularies either side of the LDS thresholds of M = 9, K = 5, D = 2
    for V, arith, mode in itertools.product((1412, 1413, 1622, 1623, 3048, 3049, 3257, 3258, 3833, 3834, 7668, 7669), ("f64", "f32", "all-fp32"), (0, 3)):
        shapes.append(dict(shape(5, 32, 300, arith, V, 0, mode), M=9, D=2))
    return shapes


def test_the_table_agrees_with_the_python_restatement_on_both_sides_of_every_threshold(table):
    shapes = _sweep()
    for key, vals in (("K", KS), ("n", NS), ("V", VS), ("rows_form", (0, 1)), ("predict_mode", range(5)), ("hyper_tn", (0, 1))):
        assert {s[key] for s in shapes} >= set(vals), key
    assert {(s["M"] + 31) // 32 * 32 for s in shapes} == set(MPS) and {s["n_cap"] // s["n"] for s in shapes} == {1, 2}
    rows = _run(table, shapes)
    bad = [(s, {k: (row[k], ref[k]) for k in row if row[k] != ref[k]}) for s, row, ref in zip(shapes, rows, map(FR.forms, shapes)) if row != ref]
    assert not bad, (len(bad), bad[:5])
    # the sweep reaches every form of every named slot
    for slot, names in Engine.FORM_NAMES.items():
        assert {row[slot] for row in rows} >= set(range(1, len(names) + 1)), slot


def test_the_highest_code_of_each_slot_is_the_number_of_its_names(table):
    out = subprocess.run([table, "max"], capture_output=True, text=True, check=True).stdout.split()
    assert dict(zip(out[::2], map(int, out[1::2]))) == {slot: len(names) for slot, names in Engine.FORM_NAMES.items()}


# ---- the M x M products of step_finish ---------------------------------------------------------------------------------------------------

MM_MPS = list(range(32, 1025, 32))
MM_ARRAYS = {"F32": (4, 8), "F64": (8, 8), "PURE": (4, 4)}       # (esz of the arrays, ssz of the solve)
DIRECT, SPLIT8 = 1, 2


def _mm(table, cases):
    """mm_plan of the program for (Mp, esz, ssz, batch, beside_chain) cases: (form, slices, reduction indices per slice) each"""
    out = subprocess.run([table, "mm"], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [tuple(map(int, row.split())) for row in out]


def test_mm_plan_against_the_restatement_and_at_the_edges_of_its_gate(table):
    cases = [(Mp, esz, ssz, batch, beside) for Mp in MM_MPS for esz, ssz in ((4, 4), (4, 8), (8, 8)) for batch in (1, 2, 4, 10, 128) for beside in (0, 1)]
    got = dict(zip(cases, _mm(table, cases)))
    bad = {c: (g, FR.mm_plan(c[0], c[1], c[3], FR.mm_tiles(c[0], c[1]), 8 * c[0] * c[0] * c[2], bool(c[4]))) for c, g in got.items()}
    bad = {c: v for c, v in bad.items() if v[0] != v[1]}
    assert not bad, (len(bad), list(bad.items())[:5])
    split = lambda Mp, esz, batch=1, beside=0: got[(Mp, esz, 8, batch, beside)]
    # float: eight slices of whole 32-deep chunks - Mp a multiple of 256
    assert [Mp for Mp in MM_MPS if split(Mp, 4)[0] == SPLIT8] == [256, 512, 768, 1024]
    assert split(256, 4) == (SPLIT8, 8, 32) and split(512, 4) == (SPLIT8, 8, 64)
    assert all(split(Mp, 4) == (DIRECT, 1, 0) for Mp in (224, 288, 384))
    # double: 16-deep chunks - every multiple of 128 from 256
    assert [Mp for Mp in MM_MPS if split(Mp, 8)[0] == SPLIT8] == list(range(256, 1025, 128))
    assert split(256, 8) == (SPLIT8, 8, 32) and split(384, 8) == (SPLIT8, 8, 48) and split(512, 8) == (SPLIT8, 8, 64)
    assert all(split(Mp, 8) == (DIRECT, 1, 0) for Mp in (128, 224, 288, 320))
    # a batch is never split, nor a product beside the chain
    assert all(g == (DIRECT, 1, 0) for c, g in got.items() if c[3] >= 2 or c[4])
    assert any(g[0] == SPLIT8 for c, g in got.items() if c[1] == 4 and c[2] == 4)


def _shared_slab(rows):
    """The cases (Mp, arrays, K, whiten) of `rows` {case: (mm_chain, mm_sbar)} in which the product beside the chain and the chain's products both go
    through the context's slab buffer.  Unwhitened, Sbar runs behind the chain on the same stream: nothing is beside it."""
    return sorted(c for c, (chain, sbar) in rows.items() if c[3] and chain == SPLIT8 and sbar == SPLIT8)


MM_CASES = [(Mp, a, K, w) for Mp in MM_MPS for a in MM_ARRAYS for K in (1, 2, 10) for w in (0, 1)]


def test_the_product_beside_the_chain_never_shares_the_chains_slab(table):
    shapes = [dict(FR.resolve(1000, Mp, K, 12, whiten=bool(w)), esz=MM_ARRAYS[a][0], ssz=MM_ARRAYS[a][1], split=0) for Mp, a, K, w in MM_CASES]
    rows = _run(table, shapes)
    prog = {c: (r["mm_chain"], r["mm_sbar"]) for c, r in zip(MM_CASES, rows)}
    ref = {c: FR.mm_forms(c[0], *MM_ARRAYS[c[1]], c[2], not c[3]) for c in MM_CASES}
    assert prog == ref
    assert _shared_slab(prog) == []
    # what the plan keeps: the chain splits wherever it did, Sbar still splits where it runs alone (K = 1, unwhitened), and K >= 2 is direct
    assert all((chain == SPLIT8) == (Mp >= 256 and Mp % (256 if MM_ARRAYS[a][1] == 4 else 128) == 0) for (Mp, a, K, w), (chain, _) in prog.items())
    assert all((sbar == SPLIT8) == (K == 1 and not w and Mp >= 256 and Mp % (256 if MM_ARRAYS[a][0] == 4 else 128) == 0)
               for (Mp, a, K, w), (_, sbar) in prog.items())


def test_the_slab_invariant_sees_the_old_rule():
    """Simulated fault: the rule as it stood (a single product splits whichever stream it runs on).  At K = 1 the whitened Sbar product and the
    chain then share the slab at exactly the sizes at which both split; K >= 2 and the unwhitened form never did."""
    old = {c: FR.mm_forms(c[0], *MM_ARRAYS[c[1]], c[2], not c[3], plan=FR.mm_plan_old) for c in MM_CASES}
    shared = _shared_slab(old)
    assert shared and all(K == 1 and w for _, _, K, w in shared)
    at = {a: [Mp for Mp, b, _, _ in shared if b == a] for a in MM_ARRAYS}
    assert at == {"F32": [256, 512, 768, 1024], "F64": list(range(256, 1025, 128)), "PURE": [256, 512, 768, 1024]}
    assert _shared_slab({c: FR.mm_forms(c[0], *MM_ARRAYS[c[1]], c[2], not c[3]) for c in MM_CASES}) == []
