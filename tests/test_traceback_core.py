"""CPU: the traceback contract (include/seqalign_hip.h, "alignments for chosen pairs") through the code the kernels share with the
host -- sequencealigner_amd/csrc/sa_traceback_core.h: the record of a cell, its scratch offset, one step of the walk, the
run-length emitter, the mirror for a > b -- compiled with g++ -fsanitize=address,undefined into tests/host_c/traceback_test.
The harness fills full tables with the reference's recurrences, records every cell through the core, walks the records through
the core and compares with a separate literal implementation of the contract over the full tables (both orders of every
pair); it also re-scores every CIGAR by the documented rule."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
NW, GA, SW = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("traceback_core") / "traceback_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "traceback_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    m = re.search(r"traceback ok: (\d+) pairs x 2 orders, (\d+) cells, (\d+) cells with a tie, (\d+) empty, (\d+) runs", res.stdout)
    assert m, res.stdout
    return dict(zip(("pairs", "cells", "ties", "empty", "runs"), map(int, m.groups())))


# method, pairs, longest, residue codes, gap / open, extend
@pytest.mark.parametrize("method,pairs,maxlen,alphabet,g1,g2", [
    (NW, 300, 90, 20, 4, 0),      # random pairs
    (GA, 300, 90, 20, 10, 1),
    (SW, 300, 90, 20, 10, 1),
    (NW, 60, 200, 4, 2, 0),       # four letters, cheap gaps, up to four strips: ties everywhere
    (GA, 60, 200, 4, 3, 1),
    (SW, 60, 200, 4, 3, 1),
    (GA, 200, 60, 20, 4, 4),      # open == extend
    (SW, 200, 60, 20, 4, 4),
    (GA, 200, 60, 20, 0, 0),      # open 0 / extend 0
    (SW, 200, 60, 20, 0, 0),
    (NW, 200, 60, 20, 0, 0),
    (GA, 200, 60, 20, 3, 7),      # |open| < |extend|: a gap is re-opened rather than extended
    (SW, 200, 60, 20, 2, 5),
    (NW, 50, 1, 20, 4, 0),        # length 1 only
    (GA, 50, 1, 20, 10, 1),
    (SW, 50, 1, 20, 10, 1),
])
def test_core_walk_equals_the_literal_contract(method, pairs, maxlen, alphabet, g1, g2, harness):
    got = run(harness, method, 1000 * method + 7 * maxlen + g1, pairs, maxlen, alphabet, g1, g2)
    assert got["pairs"] == pairs and got["runs"] > 0
    if method == SW and alphabet >= 4 and pairs > 4:
        assert got["empty"] >= 2  # the pair without a positive cell, in both orders


@pytest.mark.parametrize("method,g1,g2", [(NW, 3, 0), (GA, 3, 1), (SW, 3, 1), (GA, 2, 2), (SW, 0, 0)])
def test_homopolymers_where_every_tie_exists(method, g1, g2, harness):
    got = run(harness, method, 99 + method, 80, 150, 1, g1, g2)
    if method != SW or g1 == 0:  # (SW with costly gaps: the diagonal of matches beats every gap, the ties are in the end cell)
        assert got["ties"] > got["cells"] // 4, got
