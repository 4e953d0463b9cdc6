"""CPU: the host-compilable core of the search (sequencealigner_amd/csrc/sa_search_core.h -- segment bounds and counts, the
offsets of a query batch in its bounded packed range, the serial part + merge selection of the hits) compiled with
g++ -fsanitize=address,undefined into a stand-alone program (tests/host_c/search_core_test.cpp) and run on the host.  The
kernels (csrc/sa_search.hip: sa_k_hits_part, sa_k_hits_merge) cut the rows by the same bounds and insert by the same key.
Contract (include/seqalign_hip.h): score descending, then database index ascending; the expectation is std::partial_sort."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

NS = (1, 63, 64, 65, 1000)
SPREADS = (1, 3, 1000)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_core") / "search_core_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "search_core_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


@pytest.mark.parametrize("n", NS)
def test_part_and_merge_equal_partial_sort(n, harness):
    """every (k, S, spread) of k in {1, 7, min(N, 64)}, S in {1, 2, 5, N}, spread in {1, 3, 1000} for this N"""
    for k in sorted({1, min(7, n), min(n, 64)}):
        for s in sorted({1, 2, 5, n}):
            for spread in SPREADS:
                out = run(harness, "--select", n, k, s, spread)
                m = re.search(r"select ok: 6 rows, N = (\d+), k = (\d+), S = (\d+), (\d+) rows with a tie across the cut", out)
                assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n, k, s), out
                if spread == 1 and k < n:  # every score equal: all rows tie across the cut, the index alone decides
                    assert int(m.group(4)) == 6, out


def test_segment_bounds_cover_the_row_once(harness):
    assert "segments ok" in run(harness, "--segments")


def test_segment_counts(harness):
    assert "counts ok" in run(harness, "--counts")


def test_batch_offsets_in_the_bounded_range(harness):
    assert "offsets ok" in run(harness, "--offsets")
