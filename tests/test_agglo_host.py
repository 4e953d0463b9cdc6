"""CPU: what complete / average linkage does without a device -- sa_agglo_scratch_bytes, sa_agglo_labels through the binding
(validation, errors through sa_last_error with nothing written), the refusals the library makes before it looks for a device
(a bad method, both quantities at once, too many sequences for the int64 sums), and the tool's --linkage-method option errors."""
import subprocess

import numpy as np
import pytest

from tests.agglo_ref import AVERAGE, COMPLETE, agglo_numpy, labels_of
from tests.host_binding import ROOT
from tests.linkage_ref import random_full

POISON = -0x5A5A5A5B


def test_scratch_bytes(sa):
    for n in (2, 3, 65, 700, 10000):
        c, a = sa.agglo_scratch_bytes(n, "complete"), sa.agglo_scratch_bytes(n, "average")
        assert c == sa.agglo_scratch_bytes(n, 1) and a == sa.agglo_scratch_bytes(n, 2)
        assert 4 * n * n < c <= 4 * n * n + 64 * n + 64 and 8 * n * n < a <= 8 * n * n + 64 * n + 64  # the square matrix + O(N)
        assert c % 4 == 0 and a % 4 == 0
    assert sa.agglo_scratch_bytes(131072, 2) > 8 * 131072**2 and sa.agglo_scratch_bytes(131073, 2) == 0
    assert sa.agglo_scratch_bytes(131073, 1) > 4 * 131073**2
    for n, method in ((1, 1), (0, 2), (-7, 1), (700, 0), (700, 3), (700, -1)):
        assert sa.agglo_scratch_bytes(n, method) == 0
    with pytest.raises(sa.AlignError, match="neither 'complete' nor 'average'"):
        sa.agglo_scratch_bytes(700, "single")


@pytest.mark.parametrize("method", [COMPLETE, AVERAGE])
@pytest.mark.parametrize("n,spread", [(2, 1), (17, 3), (130, 1000), (300, 5)])
def test_labels_of_a_reference_tree(n, spread, method, sa):
    full = random_full(n, spread, 7 * n + spread)
    pairs, score = agglo_numpy(full, method)
    for t in sorted({int(score.min()) - 1, int(score.min()), int(np.median(score)), int(score.max()), int(score.max()) + 1, -2**31, 2**31 - 1}):
        want, want_clusters = labels_of(pairs, score, n, t)
        labels, clusters = sa.agglo_labels(pairs, score, n, t)
        assert labels.dtype == np.int32 and labels.shape == (n,) and clusters == want_clusters and np.array_equal(labels, want), t


def test_one_sequence_is_one_cluster(sa):
    labels, clusters = sa.agglo_labels(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 1, 0)
    assert labels.tolist() == [0] and clusters == 1


GOOD_PAIRS, GOOD_SCORE = [[2, 3], [0, 1], [0, 2], [0, 4]], [9, 9, 4, -3]  # (equal scores in descending packed index)


@pytest.mark.parametrize("pairs,score,message", [
    ([[0, 1], [1, 2], [0, 2], [3, 4]], [9, 8, 7, 6], "cycle"),
    ([[1, 0], [2, 3], [1, 2], [3, 4]], GOOD_SCORE, "lo < hi"),
    ([[0, 1], [2, 3], [1, 2], [3, 5]], GOOD_SCORE, "out of range"),
    ([[0, 1], [-1, 3], [1, 2], [3, 4]], GOOD_SCORE, "out of range"),
    (GOOD_PAIRS, [9, 9, 4, 5], "scores increase"),
    (GOOD_PAIRS, [-2**31, -2**31, -2**31, 1 - 2**31], "scores increase"),
])
def test_trees_that_are_none_fail_with_nothing_written(pairs, score, message, sa):
    lib = sa.load_library()
    n = 5
    p, s = np.array(pairs, np.int32), np.array(score, np.int32)
    out = np.full(n, POISON, np.int32)
    with pytest.raises(sa.AlignError, match=message):
        sa.agglo_labels(p, s, n, 0)
    assert lib.sa_agglo_labels(p.ctypes.data, s.ctypes.data, n, 0, out.ctypes.data) < 0 and (out == POISON).all()
    # ... and the process goes on working; the single-linkage reader rightly refuses this order of equal scores
    labels, clusters = sa.agglo_labels(GOOD_PAIRS, GOOD_SCORE, n, 5)
    assert labels.tolist() == [0, 0, 2, 2, 4] and clusters == 3
    with pytest.raises(sa.AlignError, match="order"):
        sa.linkage_labels(GOOD_PAIRS, GOOD_SCORE, n, 5)


def test_null_arguments_and_bad_sizes(sa):
    lib = sa.load_library()
    p, s = np.array(GOOD_PAIRS, np.int32), np.array(GOOD_SCORE, np.int32)
    out = np.full(5, POISON, np.int32)
    for args in ((None, s.ctypes.data, 5, 0, out.ctypes.data), (p.ctypes.data, None, 5, 0, out.ctypes.data), (p.ctypes.data, s.ctypes.data, 5, 0, None)):
        assert lib.sa_agglo_labels(*args) < 0 and b"null" in lib.sa_last_error()
    assert lib.sa_agglo_labels(p.ctypes.data, s.ctypes.data, 0, 0, out.ctypes.data) < 0 and (out == POISON).all()
    with pytest.raises(sa.AlignError, match="elements"):
        sa.agglo_labels(p[:3], s, 5, 0)
    with pytest.raises(sa.AlignError, match="int32"):
        sa.agglo_labels(p, s, 5, 2**31)


def test_the_library_refuses_before_it_looks_for_a_device(sa):
    """each of these comes back with its own message whether or not the machine has a device: none was looked for"""
    store = sa.SequenceStore.from_sequences([b"ARNDCQEG", b"ARNDCQEGHIL", b"HILKMFPSTW"])
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    with pytest.raises(sa.AlignError, match="sa_hip_agglomerate: method 0 is single linkage.*sa_hip_linkage"):
        sa.hip_agglomerate(store, scoring, 0)
    with pytest.raises(sa.AlignError, match="sa_hip_agglomerate: method 7 is neither"):
        sa.hip_agglomerate(store, scoring, 7)
    with pytest.raises(sa.AlignError, match="sa_hip_agglomerate_with_ranks: method -1 is neither"):
        sa.hip_agglomerate_with_ranks(store, scoring, -1, [0])
    with pytest.raises(sa.AlignError, match="sa_hip_agglomerate: norm and pid_denom exclude each other"):
        sa.hip_agglomerate(store, scoring, "complete", norm=sa.Norm(sa.NORM_SELF, sa.NORM_MIN), pid=sa.PID_COLUMNS)
    with pytest.raises(sa.AlignError, match="sa_hip_agglomerate_with_ranks: norm and pid_denom exclude each other"):
        sa.hip_agglomerate_with_ranks(store, scoring, "average", [0], norm=sa.Norm(sa.NORM_LENGTH, sa.NORM_MAX), pid=sa.PID_MEAN)
    with pytest.raises(sa.AlignError, match="'complete' nor 'average'"):
        sa.hip_agglomerate(store, scoring, "ward")
    many = sa.SequenceStore.from_sequences([b"AR"] * 131073)
    with pytest.raises(sa.AlignError, match="sa_hip_agglomerate: average linkage of 131073 sequences: the int64 sums hold at most 131072"):
        sa.hip_agglomerate(many, scoring, "average")
    with pytest.raises(sa.AlignError, match="rank"):  # (a bad rank: before the alignment)
        sa.hip_agglomerate_with_ranks(store, scoring, "complete", [3])


# ---- the tool's option errors ---------------------------------------------------------------------------------------------------
def cli():
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return exe


@pytest.mark.parametrize("bad,message", [
    (["--linkage-method", "complete"], "Option --linkage-method requires a tree: --linkage, --clusters, --clusters-quantile or --linkage-only"),
    (["--linkage-method", "average", "-k", "2"], "Option --linkage-method requires a tree"),
    (["--linkage", "--linkage-method", "ward"], "Linkage method must be one of single, complete, average: ward"),
    (["--linkage", "--linkage-method", ""], "Linkage method must be one of single, complete, average"),
    (["--linkage", "--linkage-method", "complete", "--linkage-method=average"], "Option --linkage-method given twice"),
    (["--linkage", "--linkage-method", "single", "--linkage-method", "single"], "Option --linkage-method given twice"),
    (["--linkage", "--linkage-method"], "Option --linkage-method requires a parameter"),
])
def test_option_errors_leave_no_output(bad, message, tmp_path):
    """refused while the options are read: before any input is loaded and before a device is looked for"""
    fasta, out = tmp_path / "in.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nARNDCQEG\n>b\nARNDCQEGHIL\n>c\nHILKMFPSTW\n")
    res = subprocess.run([str(cli()), "-i", str(fasta), "-o", str(out), "-a", "nw", "-m", "blosum62", "-p", "4", "-F", *bad],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and message in res.stderr and "usage information" in res.stderr, res.stdout + res.stderr
    assert not out.exists()


def test_help_names_the_option_and_the_promise():
    res = subprocess.run([str(cli()), "-h"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0
    assert "--linkage-method NAME" in res.stdout and "single (the default) | complete | average" in res.stdout
    assert "every pair inside a" in res.stdout and "cluster scores at least T" in res.stdout and "/linkage_method" in res.stdout
