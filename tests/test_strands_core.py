"""CPU: the host-compilable core of the two-strand search (sequencealigner_amd/csrc/sa_strands_core.h -- the IUPAC complement
table, the reverse complement of a store and its refusals, the bitmap geometry, the fold rule, the segment bounds, fold and strand
take of a row done serially) compiled with g++ -fsanitize=address,undefined into a stand-alone program
(tests/host_c/strands_test.cpp) and run on the host.  The kernels (csrc/sa_strands.hip) cut the rows by the same bounds, fold by the
same rule and read the bitmap through the same function.
Contract (include/seqalign_hip.h): a cell is reverse iff v_rev > v_fwd; the expectation is a plain loop."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

NS = (1, 63, 64, 65, 128, 129, 1000)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("strands") / "strands_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "strands_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_complement_table_is_an_involution_on_its_domain(harness):
    assert "complement ok" in run(harness, "--complement")


def test_reverse_complement_twice_is_the_identity_and_refusals_name_sequence_and_byte(harness):
    assert "rc ok" in run(harness, "--rc")


def test_segment_bounds_are_whole_words(harness):
    assert "rule ok" in run(harness, "--rule")


@pytest.mark.parametrize("n", NS)
def test_fold_and_strand_take_equal_a_plain_loop(n, harness):
    """S in {1, 2, 5, words(N)}; four kinds of content (all-tie rows and INT32_MIN / INT32_MAX cells among them) x with / without
    raw scores x in place / out of place x with / without the bitmap inside the program; tail bits zero"""
    words = (n + 63) // 64
    for s in sorted({1, min(2, words), min(5, words), words}):
        out = run(harness, "--fold", n, s)
        m = re.search(r"fold ok: N = (\d+), S = (\d+), (\d+) combinations, (\d+) reverse cells", out)
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n, s, 32), out
        assert int(m.group(4)) > 0 or n < 4  # the random kinds hold reverse cells
