"""CPU: what the search (csrc/sa_search.hip, sa_ctx_create_search) needs no device for.
  - The row bound of the launch planner (SaPlanInputs::row_end, csrc/sa_plan.cpp) compiled with g++ -fsanitize=address,undefined
    into a stand-alone program (tests/host_c/search_plan_test.cpp) and run on the stores tests/test_gpu_search.py uses: every
    (d, q) in exactly one tile or generic run, no tile with a row >= N, nq * N pairs, world = 1 refused, row_end = 0 changing
    nothing.
  - The argument checks of sa_hip_search, sa_ctx_hits, sa_hits_scratch_bytes, sa_ctx_create_search and sa_ctx_search_range that
    come before a device is looked for."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests.search_cases import MIXED_QUERY_LENGTHS
from tests.synth import make_protein_set

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "sequencealigner_amd" / "csrc"

GAPS = {"nw": (4, 0, 0), "ga": (0, 10, 1), "sw": (0, 10, 1)}


def search_lengths(n, m, seed=11):
    """lengths of the (N, M) stores of tests/test_gpu_search.py: db and queries of 20 - 60 residues"""
    return [len(s) for s in make_protein_set(n, 20, 60, seed)] + [len(s) for s in make_protein_set(m, 20, 60, seed + 1)]


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_plan") / "search_plan_test"
    tables = exe.with_name("sa_tables.o")  # (the matrix tables are data: compiled without instrumentation)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-c", str(CSRC / "sa_tables.cpp"), "-o", str(tables)])
    srcs = [ROOT / "tests" / "host_c" / "search_plan_test.cpp", CSRC / "sa_plan.cpp", CSRC / "sa_limits.cpp"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", *map(str, srcs), str(tables), "-o", str(exe)])
    return exe


def run_plan(plan_test, tmp_path, lengths, n, method, force_generic=0, no_pk=0, cus=256):
    path = tmp_path / "lens.i32"
    np.asarray(lengths, "<i4").tofile(path)
    res = subprocess.run([str(plan_test), str(path), str(n), method, "blosum62", *map(str, GAPS[method]), str(cus), str(force_generic), str(no_pk)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    assert "search plan ok" in res.stdout and "row_end = 0 ok" in res.stdout and "world = 1 refused" in res.stdout, res.stdout
    return res.stdout


@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
@pytest.mark.parametrize("n,m", [(1, 1), (3, 5), (40, 130), (700, 65)])
def test_bounded_plans_cover_the_rectangle_once(n, m, method, plan_test, tmp_path):
    out = run_plan(plan_test, tmp_path, search_lengths(n, m), n, method)
    assert f"bounded plan ok: queries [0,+{m}) x {n}" in out, out
    assert out.count("bounded plan ok") == 1 + (m > 17) + (m >= 3), out


@pytest.mark.parametrize("switch", ["force_generic", "no_pk"])
def test_bounded_plans_of_the_other_kernel_families(switch, plan_test, tmp_path):
    out = run_plan(plan_test, tmp_path, search_lengths(700, 65), 700, "nw", **{switch: 1})
    assert "bounded plan ok: queries [0,+65) x 700" in out, out
    if switch == "force_generic":  # one run per query column, nothing else
        assert "0 classes, 0 bundles, 65 generic runs" in out, out
    else:
        assert "0 bundles" in out and "0 generic runs" in out, out


def test_bounded_plan_of_mixed_column_lengths(plan_test, tmp_path):
    """8-lane, 16-lane, s32 and strip-mined columns in one store"""
    lengths = [len(s) for s in make_protein_set(300, 20, 60, 11)] + list(MIXED_QUERY_LENGTHS)
    out = run_plan(plan_test, tmp_path, lengths, 300, "nw")
    assert "bounded plan ok: queries [0,+12) x 300" in out, out


def test_a_small_device_changes_no_coverage(plan_test, tmp_path):
    """fewer CUs -> other chunk sizes, small-tile classes (j_small) from the bounded pair counts"""
    for cus in (1, 8):
        run_plan(plan_test, tmp_path, search_lengths(700, 65), 700, "nw", cus=cus)


# ---- argument checks that come before a device is looked for ------------------------------------------------------------------
def test_hits_scratch_bytes(sa):
    assert sa.hits_scratch_bytes(70, 3000, 7) == 0  # the rows alone fill the device
    assert sa.hits_scratch_bytes(200_000, 2, 64) == 8 * 2 * (200_000 // 256) * 64  # 4 k candidates per segment at least
    assert sa.hits_scratch_bytes(200_000, 2, 1) == 8 * 2 * 1024 * 1
    assert sa.hits_scratch_bytes(65, 3, 7) == 8 * 3 * 2 * 7
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0), (5, 1, 6), (100, 1, 65), (-1, 1, 1)):
        assert sa.hits_scratch_bytes(*bad) == 0


def test_bad_calls_are_refused_before_a_device_is_looked_for(sa):
    lib = sa.load_library()
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    db = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    queries = sa.SequenceStore.from_sequences(make_protein_set(3, 8, 12, 4))
    empty = sa.SequenceStore.from_sequences([])
    for k in (0, -1, 6, 65, 2 ** 31 - 1):
        with pytest.raises(sa.AlignError, match=r"k must be in \[1, min\(N, 64\)\]"):
            sa.hip_search(db, queries, scoring, k=k)
    for a, b in ((empty, queries), (db, empty)):
        with pytest.raises(sa.AlignError, match="empty store"):
            sa.hip_search(a, b, scoring, k=1)
        with pytest.raises(sa.AlignError, match="empty store"):
            sa.SearchContext(a, b, scoring)
    with pytest.raises(sa.AlignError, match="nothing asked for"):
        sa.hip_search(db, queries, scoring)
    sc = scoring._as_c()
    index, score = np.full(9, 77, np.int32), np.full(9, 77, np.int32)
    assert not lib.sa_hip_search(db._as_c(), queries._as_c(), None, 3, index.ctypes.data, score.ctypes.data, None) and b"null" in lib.sa_last_error()
    assert not lib.sa_hip_search(db._as_c(), queries._as_c(), C.byref(sc), 3, index.ctypes.data, None, None) and b"go together" in lib.sa_last_error()
    assert not lib.sa_hip_search(db._as_c(), queries._as_c(), C.byref(sc), 3, None, None, None) and b"nothing asked for" in lib.sa_last_error()
    null_store = sa.binding._Input(None, None, 0, 5)
    assert not lib.sa_hip_search(null_store, queries._as_c(), C.byref(sc), 3, index.ctypes.data, score.ctypes.data, None) and b"null" in lib.sa_last_error()
    assert not lib.sa_ctx_create_search(0, db._as_c(), queries._as_c(), None) and b"null scoring" in lib.sa_last_error()
    assert lib.sa_ctx_hits(None, None, 1, 1, None, None, None, None) != 0 and b"null context" in lib.sa_last_error()
    assert lib.sa_ctx_search_range(None, 0, 1, None, None, None) != 0 and b"null context" in lib.sa_last_error()
    assert lib.sa_search_scratch_bytes(None, 0, 1) == 0
    assert lib.sa_ctx_search_db(None) == 0 and lib.sa_ctx_search_queries(None) == 0
    assert (index == 77).all() and (score == 77).all()
