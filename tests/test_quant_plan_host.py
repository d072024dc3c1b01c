"""CPU tests of the quantile mode's planning rule (gdrf_amd/csrc/forms.h::quant_plan): the header is compiled with the host compiler
into the table program tests/host/quant_plan.cpp, as tests/test_forms_host.py builds its own, and compared with the Python restatement
of tests/_quant_ref.py over both sides of every sample, topic and component edge."""
import os
import shutil
import subprocess

import pytest

from tests import _quant_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128)
SS = (1, 2, 255, 256, 257, 1024)
ESZ = (4, 8)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """the table program, built once; no compiler is a failure, not a skip"""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm if os.path.exists(rocm) else None)
    assert cxx, "no host C++ compiler: neither c++ on PATH nor ROCm's clang++"
    exe = str(tmp_path_factory.mktemp("quant") / "quant_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "quant_plan.cpp")], check=True)
    return exe


def _run(table, shapes):
    """[(RP, CP, P, lds)] of the shapes (K, C, S, esz, LG)"""
    out = subprocess.run([table], input="".join(" ".join(map(str, s)) + "\n" for s in shapes), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(shapes)
    return [tuple(int(v) for v in line.split()) for line in out]


def _sweep():
    return [(K, C, S, esz, QR.lane_group(K)) for K in KS for C in sorted({1, K, 50, 4096}) for S in SS for esz in ESZ]


def test_the_budget_is_the_restatements(table):
    assert int(subprocess.run([table, "budget"], capture_output=True, text=True, check=True).stdout) == QR.QUANT_LDS <= 150 * 1024


def test_the_plan_equals_the_restatement_and_fits_on_the_whole_sweep(table):
    shapes = _sweep()
    seen = dict(fewer_rows=0, one_row=0, ragged=0, single_pass=0)
    for (K, C, S, esz, LG), (RP, CP, P, lds) in zip(shapes, _run(table, shapes)):
        assert (RP, CP, lds) == QR.quant_plan(K, C, S, esz, LG), (K, C, S, esz)
        assert P >= S and P & (P - 1) == 0 and (P == 1 or P // 2 < S), (S, P)
        assert lds <= QR.QUANT_LDS and 1 <= RP <= 256 // LG and 1 <= CP <= C, (K, C, S, esz, RP, CP, lds)
        seen["fewer_rows"] += RP < 256 // LG
        seen["one_row"] += RP == 1
        seen["ragged"] += CP < C and C % CP != 0
        seen["single_pass"] += RP == 256 // LG and CP == C
    print(seen)
    assert all(seen.values()), seen


def test_the_gpu_cases_that_name_a_plan_reach_it(table):
    shapes = [(K, K, S, esz, QR.lane_group(K)) for (K, S, esz) in QR.GPU_PLANS]
    for key, (RP, CP, _, lds) in zip(QR.GPU_PLANS, _run(table, shapes)):
        assert (RP, CP, lds) == QR.GPU_PLANS[key], key
    K, S, esz = 8, 1024, 8                  # one end: the samples of one component of a row take 8 KB, not every group gets a row
    assert QR.GPU_PLANS[(K, S, esz)][0] < 256 // QR.lane_group(K) and QR.GPU_PLANS[(K, S, esz)][1] == 1
    for esz in ESZ:                          # the other: four groups, several components of 128 per pass and a ragged last pass
        RP, CP, _ = QR.GPU_PLANS[(128, 1024, esz)]
        assert RP <= 4 and 1 < CP < 128 and 128 % CP != 0
