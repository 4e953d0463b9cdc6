"""CPU: the two forms of the complete- / average-linkage expectation (tests/agglo_ref.py) agree with each other, and the fast
one agrees with scipy.cluster.hierarchy.linkage on a matrix without ties.  Nothing here runs the code under test."""
import numpy as np
import pytest

from tests.agglo_ref import AVERAGE, COMPLETE, agglo_fractions, agglo_numpy, labels_of, merge_table, tie_free_full
from tests.linkage_ref import random_full

METHOD_IDS = {COMPLETE: "complete", AVERAGE: "average"}


@pytest.mark.parametrize("method", [COMPLETE, AVERAGE], ids=METHOD_IDS.get)
@pytest.mark.parametrize("spread", [1, 3, 1000])
@pytest.mark.parametrize("n", [2, 3, 16, 17, 40])
def test_the_two_forms_agree(n, spread, method):
    full = random_full(n, spread, 1000 * n + spread)
    slow, fast = agglo_fractions(full, method), agglo_numpy(full, method)
    for a, b in zip(slow, fast):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    pairs, score = fast
    assert pairs.shape == (n - 1, 2) and score.shape == (n - 1,)
    assert (pairs[:, 0] < pairs[:, 1]).all()
    assert (np.diff(score.astype(np.int64)) <= 0).all(), "score increases"
    assert merge_table(pairs, n)[-1, 2] == n  # (a spanning tree: the union-find asserts that no pair closes a cycle)
    if spread == 1:
        assert pairs.tolist() == [[0, t + 1] for t in range(n - 1)]


def test_extreme_values_stay_exact():
    n = 17
    rng = np.random.default_rng(3)
    m = np.triu(rng.choice(np.array([-2**31, -1, 0, 2**31 - 1], np.int64), size=(n, n)), 1)
    full = (m + m.T).astype(np.int32)
    for method in (COMPLETE, AVERAGE):
        slow, fast = agglo_fractions(full, method), agglo_numpy(full, method)
        assert np.array_equal(slow[0], fast[0]) and np.array_equal(slow[1], fast[1])


@pytest.mark.parametrize("method", [COMPLETE, AVERAGE], ids=METHOD_IDS.get)
def test_tie_free_matrix_equals_scipy(method):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    n = 300
    full = tie_free_full(n, 5)
    tri = full[np.triu_indices(n, 1)]
    assert np.unique(tri).size == tri.size
    pairs, score = agglo_numpy(full, method)
    assert (np.diff(score.astype(np.int64)) <= 0).all()
    dist = -full.astype(np.float64)
    np.fill_diagonal(dist, 0.0)
    z = hierarchy.linkage(squareform(dist, checks=False), METHOD_IDS[method])
    table = merge_table(pairs, n)
    assert np.array_equal(table[:, :2], z[:, :2].astype(np.int64)) and np.array_equal(table[:, 2], z[:, 3].astype(np.int64))
    assert np.array_equal(score, np.floor(-z[:, 2]).astype(np.int64))  # (heights: the floor of the exact average)


def test_labels_are_a_prefix_of_the_merges():
    full = random_full(40, 1000, 9)
    pairs, score = agglo_numpy(full, COMPLETE)
    for t in (int(score.max()) + 1, int(score.max()), int(np.median(score)), int(score.min()), int(score.min()) - 1):
        labels, clusters = labels_of(pairs, score, 40, t)
        assert clusters == 40 - int((score >= t).sum()) == np.unique(labels).size
        same = labels[:, None] == labels[None, :]
        np.fill_diagonal(same, False)
        assert (full[same] >= t).all(), "complete linkage: a pair inside a cluster scores below the threshold"
