"""CPU: the rules that pick a kernel form per stage (gdrf_amd/csrc/forms.h), checked without a GPU through the stand-alone table program
tests/host/forms_table.cpp, built once per session with the host compiler.

1. Every case of the four GPU form tests (their own tables: SHAPES of test_gpu_wbar_w1 and test_gpu_fwd_t_w1, CASES of test_gpu_topic_forms,
   GROUPS of _predict_ref) still reaches the form it asserts on the GPU, so a change of a threshold shows here and not only on a GPU.
2. A sweep with both sides of every threshold against tests/_forms_ref.py, an independent Python statement of the rules: every slot and the
   split counts of A_k, G^T and the hyper-TN form.
3. The highest code of each named slot is the number of names Engine.FORM_NAMES has for it."""
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
    from tests import test_gpu_fwd_t_w1, test_gpu_topic_forms, test_gpu_wbar_w1
    cases = []
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
                    predict_mode=mode)

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
