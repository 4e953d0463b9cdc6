"""CPU: the contract of the score graph (sequencealigner_amd/csrc/sa_edges_core.h -- the predicate, the packed index of a row's
two pieces, the serial count, scan and fill) compiled with g++ -fsanitize=address,undefined into tests/host_c/edges_test and
run on the host: the kernels (csrc/sa_edges.hip) use the same predicate and index arithmetic and place every entry where the
serial fill places it.  Contract (include/seqalign_hip.h): score(r, c) >= min_score, c != r, columns ascending per row."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("edges_core") / "edges_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "edges_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_piece_index_and_predicate(harness):
    """c < r and c > r land on the definition's packed index up to N = 300 000 (64-bit), runs are contiguous, >= is >="""
    assert "index ok" in run(harness, "--index")


@pytest.mark.parametrize("spread", [1, 3, 1000])  # all equal; heavy repeats (the threshold occurs often); few repeats
@pytest.mark.parametrize("n", [2, 3, 16, 17, 64, 65, 130])
def test_serial_count_and_fill_equal_the_double_loop(n, spread, harness):
    out = run(harness, "--graph", 1000 * n + spread, n, spread)
    m = re.search(r"graph ok: (\d+) rows, 7 thresholds, (\d+) edges compared, (\d+) empty rows met", out)
    assert m and int(m.group(1)) == n, out
    assert int(m.group(2)) >= 3 * n * (n - 1)  # below the minimum, at it or INT32_MIN: every off-diagonal entry, three times
    assert int(m.group(3)) >= 2 * n            # above the maximum and INT32_MAX: every row empty
