"""CPU tests of log(w!) as the per-row predictive score forms its Multinomial coefficient (gdrf_amd/csrc/score_lfact.h): the header is
compiled with the host compiler into the table program tests/host/score_lfact.cpp, as tests/test_quant_plan_host.py builds its own.

Bound.  The table holds correctly rounded logs of exact factorials; above it Stirling's series is cut where its first omitted term is
below 3e-16 of the value, and its evaluation rounds a handful of times with a cancellation factor (x log x) / (x log x - x) of at most
1.5 (at x = 25).  The references - Python's math.log of the exact integer factorial and math.lgamma - are good to an ulp or a few.  Both
together stay well inside BOUND = 16 ulps of the value, 3.6e-15; the GPU tests hold log_coef, a sum of these, to 1e-9 only."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 16 * 2.0 ** -52


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """the table program, built once; no compiler is a failure, not a skip"""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm if os.path.exists(rocm) else None)
    assert cxx, "no host C++ compiler: neither c++ on PATH nor ROCm's clang++"
    exe = str(tmp_path_factory.mktemp("lfact") / "score_lfact")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "score_lfact.cpp")], check=True)
    return exe


def lfact(table, ws):
    out = subprocess.run([table], input="".join(f"{float(w)!r}\n" for w in ws), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(ws)
    return [float(v) for v in out]


def exact(w):
    """log(w!) from the exact integer factorial"""
    return math.log(math.factorial(w))


def test_the_table_holds_the_logs_of_the_exact_factorials(table):
    n = int(subprocess.run([table, "table"], capture_output=True, text=True, check=True).stdout)
    assert n == 24
    got = lfact(table, range(n))
    assert got[0] == 0.0 and got[1] == 0.0                  # 0! = 1! = 1: exactly nothing, so a row of ones has log_coef = log(total!)
    for w in range(2, n):
        assert abs(got[w] - exact(w)) <= 2.0 ** -52 * exact(w), (w, got[w], exact(w))


def test_the_series_takes_over_from_the_table_without_a_step(table):
    ws = [22, 23, 24, 25, 26]                              # 23 is the last entry of the table, 24 the first count of the series
    got = lfact(table, ws)
    for w, v in zip(ws, got):
        assert abs(v - exact(w)) <= BOUND * exact(w), (w, v, exact(w))
    for (w, a), b in zip(zip(ws, got), got[1:]):           # log((w + 1)!) - log(w!) = log(w + 1), across the switch as beside it
        assert abs((b - a) - math.log(w + 1)) <= 2 * BOUND * b, w


def test_every_count_below_1e5_and_a_sample_of_larger_ones_against_lgamma(table):
    ws = list(range(100_000)) + [100_000 + 997 * i for i in range(3000)] + [10 ** 7, 10 ** 9, 2 ** 31 - 1, 2 ** 31, 10 ** 12, 10 ** 15]
    worst = 0.0
    for w, v in zip(ws, lfact(table, ws)):
        want = math.lgamma(w + 1.0)
        err = abs(v - want) / want if want else abs(v)
        worst = max(worst, err)
        assert err <= BOUND, (w, v, want)
    print(f"largest relative difference to lgamma: {worst:.3e}")
    big = [100, 1000, 9999, 10000, 65536, 100_000]          # and against the exact factorial where that is quick to form
    for w, v in zip(big, lfact(table, big)):
        assert abs(v - exact(w)) <= BOUND * exact(w), (w, v, exact(w))


def test_what_is_no_count_reads_as_an_absent_entry(table):
    assert lfact(table, [-1, -3, -1e9, 0.5]) == [0.0, 0.0, 0.0, 0.0]
