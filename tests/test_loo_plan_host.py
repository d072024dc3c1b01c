"""CPU tests of the PSIS leave-one-out planning rule (gdrf_amd/csrc/forms.h::loo_plan): the header is compiled with the host compiler
into the table program tests/host/loo_plan.cpp, as tests/test_quant_plan_host.py builds its own, and compared with the Python restatement
of tests/_loo_ref.py over both sides of every topic, sample and vocabulary edge, both element sizes, dense and CSR."""
import os
import shutil
import subprocess

import pytest

from tests import _loo_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128)
SS = (25, 64, 65, 256, 257, 1024)
VS = (1, 128, 129, 4096)
ESZ = (4, 8)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """the table program, built once; no compiler is a failure, not a skip"""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm if os.path.exists(rocm) else None)
    assert cxx, "no host C++ compiler: neither c++ on PATH nor ROCm's clang++"
    exe = str(tmp_path_factory.mktemp("loo") / "loo_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "loo_plan.cpp")], check=True)
    return exe


def _run(table, shapes):
    """[(RP, P, M, stride, lds)] of the shapes (K, V, S, esz, LG, csr)"""
    out = subprocess.run([table], input="".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) == len(shapes)
    return [tuple(int(v) for v in line.split()) for line in out]


def test_the_budgets_are_the_restatements(table):
    rows, cu, wgs, stage = (int(v) for v in subprocess.run([table, "budget"], capture_output=True, text=True, check=True).stdout.split())
    assert (rows, cu, wgs, stage) == (LR.LDS_ROWS, LR.LDS_MAX, LR.WG_CU, LR.STAGE_WG_CU) and rows == 150 * 1024 <= cu


def test_the_plan_equals_the_restatement_and_fits_on_the_whole_sweep(table):
    shapes = [(K, V, S, esz, LR.lane_group(K), csr) for K in KS for V in VS for S in SS for esz in ESZ for csr in (False, True)]
    seen = dict(every_group=0, fewer_rows=0, one_row=0)
    for (K, V, S, esz, LG, csr), got in zip(shapes, _run(table, shapes)):
        assert got == LR.loo_plan(K, V, S, esz, LG, csr), (K, V, S, esz, csr)
        RP, P, M, stride, lds = got
        assert P >= S and P & (P - 1) == 0 and P // 2 < S and M == LR.tail_len(S) and stride == P + M + 3 * LR.fit_grid(M)
        assert lds <= LR.LDS_ROWS and 1 <= RP <= 256 // LG, (K, V, S, esz, csr, RP, lds)
        Kp, W = (K + LG - 1) // LG * LG, min(V, 128)
        assert lds == (0 if csr else K * W * esz) + RP * (stride * 8 + Kp * esz + (0 if csr else W * 4))
        seen["every_group"] += RP == 256 // LG
        seen["fewer_rows"] += 1 < RP < 256 // LG
        seen["one_row"] += RP == 1
    print(seen)
    assert all(seen.values()), seen


def test_the_largest_unit_fits_with_one_row(table):
    """K = 128 in double, a full chunk of Phi, S = 1024: 128 KB of Phi, the row's 1024 + 96 + 3 x 39 doubles, 1 KB of theta, 512 B of counts"""
    (RP, P, M, stride, lds), = _run(table, [(128, 4096, 1024, 8, 64, False)])
    assert (RP, P, M, stride) == (1, 1024, 96, 1237) and lds == 128 * 128 * 8 + 1237 * 8 + 128 * 8 + 128 * 4 == 142504 <= LR.LDS_ROWS


def test_the_stage_kernels_plan(table):
    shapes = [(0, 0, S, 0, LR.PSIS_LG, True) for S in (25, 63, 64, 65, 257, 1024)]
    for (_, _, S, _, _, _), got in zip(shapes, _run(table, shapes)):
        assert got == LR.stage_plan(S) and got[4] == got[0] * got[3] * 8 <= LR.LDS_ROWS, S
    assert LR.stage_plan(25)[0] == 16 and LR.stage_plan(1024)[0] < 16
