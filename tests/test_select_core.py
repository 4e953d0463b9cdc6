"""CPU: the contract of the order statistics of the score distribution (sequencealigner_amd/csrc/sa_select_core.h -- the key, the
byte of a round, the serial count, the narrowing step, the group deduplication, the scratch layout and sa_score_rank's rule)
compiled with g++ -fsanitize=address,undefined into tests/host_c/select_test and run on the host: the kernels
(csrc/sa_select.hip) call the same functions.  Contract (include/seqalign_hip.h): value = the rank-th smallest entry, below = the
number of entries strictly below it; the expectation is std::sort's, never the code's own."""
import math
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
SIZES = [1, 2, 3, 63, 64, 65, 257, 5000]
SPREADS = ["equal", "pm", "extremes", "band", "uniform"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("select_core") / "select_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "select_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_key_bytes_and_scratch_layout(harness):
    """the key keeps the order over all of int32 and turns back, four bytes make it, the layout is 8-byte aligned"""
    assert "keys ok" in run(harness, "--keys")


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("pairs", SIZES)
def test_serial_select_equals_sort(pairs, spread, harness):
    """ranks 0, P - 1, P / 2, sixteen equal and sixteen spread ones; the groups of a round never exceed the ranks"""
    out = run(harness, "--select", 7 * pairs + len(spread), pairs, spread)
    m = re.search(r"select ok: (\d+) entries, 5 rank sets, (\d+) groups at most", out)
    assert m and int(m.group(1)) == pairs, out
    assert 1 <= int(m.group(2)) <= 16
    if spread == "equal":
        assert int(m.group(2)) == 1  # one value: every rank stays in one group
    if spread == "uniform" and pairs == 5000:
        assert int(m.group(2)) == 16  # sixteen spread ranks land in sixteen top bytes


def python_rank(pairs, q):
    """the rule of the header, in Python"""
    if pairs < 1 or math.isnan(q) or not 0.0 <= q <= 1.0:
        return -1
    return min(pairs - 1, int(q * pairs))


RANK_TABLE = [(100, 0.0), (100, 1.0), (100, 0.99), (100, 0.98), (100, 0.5), (1, 0.0), (1, 1.0), (1, 0.7), (3, 1 / 3), (3, 2 / 3), (10, 0.3),
              (4_999_950_000, 0.0), (4_999_950_000, 0.5), (4_999_950_000, 0.99), (4_999_950_000, 0.999), (4_999_950_000, 1.0),
              (2 ** 61, 1.0), (2 ** 61, 0.999999999), (49_995_000, 0.999),
              (100, float("nan")), (100, -0.1), (100, 1.5), (0, 0.5), (-3, 0.5), (100, float("inf"))]


def test_score_rank_is_the_python_rule(harness):
    # the IEEE product 0.99 * 100 is exactly 99.0 (the double nearest 0.99 lies below it, the product rounds up), so the rule gives
    # 99 = P - 1 here, not the 98 of exact arithmetic; 0.98 * 100 = 98.0 is the neighbour
    assert python_rank(100, 0.99) == 99 and python_rank(100, 0.98) == 98 and python_rank(100, 1.0) == 99 and python_rank(100, 0.0) == 0
    assert python_rank(100, float("nan")) == python_rank(100, -0.1) == python_rank(100, 1.5) == python_rank(0, 0.5) == -1
    args = []
    for pairs, q in RANK_TABLE:
        args += [pairs, repr(q), python_rank(pairs, q)]
    assert f"rank ok: {len(RANK_TABLE)} cases" in run(harness, "--rank", *args)
