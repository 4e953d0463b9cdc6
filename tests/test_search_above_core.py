"""CPU: the host-compilable core of the threshold search (sequencealigner_amd/csrc/sa_search_above_core.h -- the segment rule, the
scratch size, count / scan / fill of a row cut into segments done serially) compiled with g++ -fsanitize=address,undefined into a
stand-alone program (tests/host_c/search_above_test.cpp) and run on the host.  The kernels (csrc/sa_search_above.hip:
sa_k_above, sa_k_above_scan) cut the rows by the same bounds and place the hits from the same scanned bases.
Contract (include/seqalign_hip.h): d is a hit of row r iff vrect[r, d] >= min_value; ascending d; the expectation is a plain loop."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

NS = (1, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_above") / "search_above_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "search_above_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_segment_rule_and_scratch_size(harness):
    assert "rule ok" in run(harness, "--rule")


@pytest.mark.parametrize("n", NS)
def test_count_scan_fill_equal_a_plain_loop(n, harness):
    """S in {1, 2, 5, N}; four kinds of content x eleven thresholds (INT32_MIN and INT32_MAX among them) inside the program"""
    for s in sorted({1, 2, 5, n}):
        out = run(harness, "--csr", n, s)
        m = re.search(r"csr ok: N = (\d+), S = (\d+), (\d+) combinations, (\d+) hits", out)
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n, s, 44), out
        assert int(m.group(4)) >= 4 * 4 * n  # INT32_MIN alone keeps every candidate of every kind
