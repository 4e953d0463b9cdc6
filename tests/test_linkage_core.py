"""CPU: the contract of the single-linkage tree (sequencealigner_amd/csrc/sa_linkage_core.h -- the order predicate, the packed
index and its inverse, the root rule of a Boruvka round, the serial tree, the labels at a threshold and the merge table)
compiled with g++ -fsanitize=address,undefined into tests/host_c/linkage_test and run on the host: the kernels
(csrc/sa_linkage.hip) use the same predicate, index arithmetic and root rule.  Contract (include/seqalign_hip.h): pair e comes
before pair f iff score(e) > score(f), or the scores are equal and p(e) < p(f); the tree is the N - 1 pairs in that order."""
import math
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
SIZES = [2, 3, 16, 17, 64, 65, 130]
SPREADS = [1, 3, 1000]  # all equal; heavy ties; few ties


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("linkage_core") / "linkage_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "linkage_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_order_predicate_and_packed_index(harness):
    """a strict order with 64-bit packed indices; the index and its inverse agree with the definition up to N = 300 000"""
    assert "index ok" in run(harness, "--index")


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("n", SIZES)
def test_serial_tree_equals_kruskal(n, spread, harness):
    m = re.search(r"tree ok: (\d+) rows, (\d+) merges", run(harness, "--tree", 1000 * n + spread, n, spread))
    assert m and int(m.group(1)) == n and int(m.group(2)) == n - 1


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("n", SIZES + [300])
def test_rounds_with_the_root_rule_give_the_serial_tree(n, spread, harness):
    """mutual hooks keep the smaller id as root and record their pair once, chains end, ceil(log2 N) rounds are enough"""
    out = run(harness, "--rounds", 1000 * n + spread, n, spread)
    m = re.search(r"rounds ok: (\d+) rows, (\d+) rounds \(bound (\d+)\), (\d+) mutual hooks, deepest chain (\d+)", out)
    assert m and int(m.group(1)) == n, out
    assert 1 <= int(m.group(2)) <= int(m.group(3)) == math.ceil(math.log2(n))
    assert int(m.group(4)) >= 2  # every round has at least one mutual pair, counted from both ends
    if spread == 1:
        assert int(m.group(2)) == 1 and int(m.group(4)) == 2  # the star: everything hooks to 0 in one round, 0 and 1 mutually


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("n", SIZES)
def test_labels_and_merges_equal_the_double_loops(n, spread, harness):
    m = re.search(r"cut ok: (\d+) rows, 7 thresholds, (\d+) merges", run(harness, "--cut", 1000 * n + spread, n, spread))
    assert m and int(m.group(1)) == n and int(m.group(2)) == n - 1


def test_trees_that_are_none_are_refused_with_nothing_written(harness):
    assert "refuse ok: 7 trees" in run(harness, "--refuse")
