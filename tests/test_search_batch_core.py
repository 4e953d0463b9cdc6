"""CPU: the batch rule of the one-call search forms (sequencealigner_amd/csrc/sa_search_batch_core.h -- the device bytes of a
query for each form and kind, the budget, the queries of a batch, the tiling of [0, M)) compiled with
g++ -fsanitize=address,undefined into a stand-alone program (tests/host_c/search_batch_test.cpp) and run on the host.  The
drivers (csrc/sa_search_run.h and the five files that use it) size their batches by these functions and no others; the
expectation is the wording of include/seqalign_hip.h written out, which the GPU tests restate to force exact batch counts."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_batch") / "search_batch_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "search_batch_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_bytes_of_a_query_equal_the_header_formulas(harness):
    """the seven forms in every kind, with and without hits; N = 1, the bitmap word edge 63 / 64 / 65, k = 64"""
    assert "bytes ok: 120 (N, M, k)" in run(harness, "--bytes")


def test_batch_size_edges_and_tiling(harness):
    """budget below one query, an exact multiple and one byte less, cap 0, a cap above the free memory, M below the room"""
    assert "batches ok" in run(harness, "--batches")


def test_largest_sizes_overflow_nothing(harness):
    """N = M = 2^31 - 1, k = 64, a budget of 2^62: UBSan is the judge"""
    assert "limits ok" in run(harness, "--limits")


def test_the_drivers_keep_one_copy_of_the_rule():
    """a guard on the source text, not a test of the drivers (the GPU tests of the forms are that): the scaffolding is spelled
    once under csrc/ (sa_traceback.hip's own DevBuf<T> / Sync are another family's), so that a sixth form cannot copy it unnoticed"""
    csrc = ROOT / "sequencealigner_amd" / "csrc"
    family = ["sa_search.hip", "sa_search_quantity.hip", "sa_search_above.hip", "sa_strands.hip", "sa_fit.hip", "sa_search_run.h",
              "sa_search_batch_core.h"]
    text = {name: (csrc / name).read_text() for name in family}
    for needle in ("struct DevBuf", "struct Sync", "hipMemGetInfo(", "env.search_batch_bytes"):
        assert [name for name in family if needle in text[name]] == ["sa_search_run.h"], needle
        assert text["sa_search_run.h"].count(needle) == 1, needle
