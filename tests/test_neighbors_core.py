"""CPU: the ordering contract of the nearest-neighbour selection (sequencealigner_amd/csrc/sa_neighbors_core.h -- the 64-bit key,
the threshold / position / shift insertion, the serial per-row selection) compiled with g++ -fsanitize=address,undefined into
tests/host_c/neighbors_test and run on the host: the kernel (csrc/sa_neighbors.hip) orders by the same key and inserts in the
same three steps, one list entry per lane.  Contract (include/seqalign_hip.h): score descending, then index ascending."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("neighbors_core") / "neighbors_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "neighbors_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_key_order_is_the_contract(harness):
    """scores INT32_MIN, SA_SCORE_MIN, -1, 0, INT32_MAX ...; indices 0 .. 2^31 - 1: key order == (score desc, index asc),
    keys decode, every key is above the empty entry"""
    assert "keys ok" in run(harness, "--keys")


@pytest.mark.parametrize("n,k,spread", [
    (2, 1, 3),          # one candidate
    (40, 1, 2),         # k = 1, two distinct scores
    (40, 39, 4),        # k = N - 1: every candidate, fully sorted
    (65, 64, 5),        # k = 64 = N - 1
    (300, 64, 3),       # k = 64 with heavy ties
    (300, 7, 1),        # every score equal: index order alone
    (257, 32, 1000),    # few ties
])
def test_serial_selection_equals_partial_sort(n, k, spread, harness):
    out = run(harness, "--rows", 1000 * n + k, n, k, spread)
    m = re.search(r"rows ok: (\d+) rows, k = (\d+), (\d+) rows with a tie across the cut", out)
    assert m and int(m.group(1)) == n and int(m.group(2)) == k, out
    if spread <= 5 and k < n - 1:  # the cases meant to test the tie rule do contain ties across the cut
        assert int(m.group(3)) >= n // 2, out
