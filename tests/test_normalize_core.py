"""CPU: the contract of the normalised scores (sequencealigner_amd/csrc/sa_normalize_core.h -- the value rule with its floor
division and saturation, the deal of the triangle's columns, the packed index arithmetic) compiled with
g++ -fsanitize=address,undefined into tests/host_c/normalize_test and run on the host: the kernels (csrc/sa_normalize.hip) call
the same functions.  Contract (include/seqalign_hip.h): floor(num / D) rounded towards minus infinity, INT32_MIN for D <= 0,
saturated to int32; the expectation is __int128 arithmetic, never the code's own double quotient."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("normalize_core") / "normalize_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "normalize_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_value_over_the_grid_of_edge_values(harness):
    """s, d[i], d[j] over INT32_MIN, INT32_MIN + 1, -SCALE, -1, 0, 1, 2, 3, SCALE - 1, SCALE, SCALE + 1, INT32_MAX - 1, INT32_MAX"""
    assert f"grid ok: {13 ** 3 * 3} cases" in run(harness, "--grid")


def test_value_over_a_million_random_triples(harness):
    out = run(harness, "--random", 20261018, 1_000_000)
    m = re.search(r"random ok: 1000000 triples, (\d+) negative inexact quotients", out)
    assert m and int(m.group(1)) > 100_000, out  # (the floor rule is exercised, not only met by exact quotients)


@pytest.mark.parametrize("n", [2, 3, 65])
def test_serial_triangle_equals_the_direct_formula(n, harness):
    """the column walk and the index arithmetic: every (i, j) once, nothing beyond P written, in place gives the same bytes"""
    assert f"triangle ok: {n} sequences, {n * (n - 1) // 2} pairs" in run(harness, "--triangle", n, 11 * n)


@pytest.mark.parametrize("n", [2, 3, 4, 65, 92683, 100000])
def test_index_functions(n, harness):
    """every column dealt once, equal work per unit, 64-bit indices (P passes 2^32 at N = 92 683)"""
    out = run(harness, "--index", n)
    assert f"index ok: {n} columns, {n * (n - 1) // 2} entries, last start {(n - 1) * (n - 2) // 2}" in out
