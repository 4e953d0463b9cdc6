"""CPU: the contract of complete and average linkage (sequencealigner_amd/csrc/sa_agglo_core.h -- the order predicate with its
128-bit products, the combine rules, the floor division, the cache rule, the serial greedy tree and the labels) compiled with
g++ -fsanitize=address,undefined into tests/host_c/agglo_test and run on the host: the kernels (csrc/sa_agglo.hip) use the same
predicate, rules and cache rule, and the harness replays their steps."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
SIZES = [2, 3, 16, 17, 64, 65, 130]
SPREADS = [1, 3, 1000]  # all equal; heavy ties; few ties
METHODS = {1: "complete", 2: "average"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("agglo_core") / "agglo_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "agglo_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_order_predicate_at_the_extremes(harness):
    """S = +-(2^62 - 1), n up to 2^34; equal rationals with different terms; antisymmetric, total, transitive; the floor"""
    assert "predicate ok" in run(harness, "--predicate")


def test_index_arithmetic_and_sums_at_the_largest_n(harness):
    assert "index ok" in run(harness, "--index")


@pytest.mark.parametrize("method", METHODS, ids=METHODS.get)
@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("n", SIZES)
def test_replay_of_the_device_steps_gives_the_serial_tree(n, spread, method, harness):
    """row-best caches, pick, merge with keep-without-rescan; after every step every cache is the first of its row"""
    m = re.search(r"replay ok: (\d+) rows, (\d+) merges, (\d+) rescans", run(harness, "--replay", 1000 * n + spread, n, spread, method))
    assert m and int(m.group(1)) == n and int(m.group(2)) == n - 1
    assert int(m.group(3)) <= (n - 1) * (n - 2)
    if spread == 1:
        assert int(m.group(3)) == 0  # (all equal: the new entry never comes after the cached key)


@pytest.mark.parametrize("method", METHODS, ids=METHODS.get)
@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("n", SIZES)
def test_labels_equal_the_double_loop(n, spread, method, harness):
    m = re.search(r"cut ok: (\d+) rows, 7 thresholds, (\d+) merges", run(harness, "--cut", 1000 * n + spread, n, spread, method))
    assert m and int(m.group(1)) == n and int(m.group(2)) == n - 1


def test_trees_and_scores_that_must_be_refused(harness):
    assert "refuse ok: 7 trees" in run(harness, "--refuse")
