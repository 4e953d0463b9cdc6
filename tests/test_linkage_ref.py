"""CPU: the expectation of the single-linkage tests against itself (tests/linkage_ref.py): Prim in NumPy equals Kruskal in plain
Python under the contract's total order, the all-equal matrix gives the star from 0, and the labels of a cut tree are the
components of the thresholded matrix."""
import numpy as np
import pytest

from tests.linkage_ref import kruskal_tree, labels_at, prim_tree, random_full


@pytest.mark.parametrize("spread", [1, 3, 1000])  # all equal; heavy ties; few ties
@pytest.mark.parametrize("n", [2, 3, 17, 65, 130, 300])
def test_prim_equals_kruskal(n, spread):
    full = random_full(n, spread, 1000 * n + spread)
    pairs, score = prim_tree(full)
    want_pairs, want_score = kruskal_tree(full)
    assert pairs.dtype == np.int32 and pairs.shape == (n - 1, 2) and score.dtype == np.int32 and score.shape == (n - 1,)
    assert np.array_equal(pairs, want_pairs) and np.array_equal(score, want_score)
    assert (pairs[:, 0] < pairs[:, 1]).all() and (np.diff(score.astype(np.int64)) <= 0).all()


@pytest.mark.parametrize("n", [2, 66, 130])
@pytest.mark.parametrize("value", [7, -2**31, 2**31 - 1])
def test_all_equal_gives_the_star_from_0(n, value):
    full = np.full((n, n), value, np.int32)
    pairs, score = prim_tree(full)
    assert pairs.tolist() == [[0, j] for j in range(1, n)] and (score == value).all()


def test_cut_tree_is_the_thresholded_graph():
    n = 130
    full = random_full(n, 40, 5)
    pairs, score = prim_tree(full)
    for t in sorted(set(score.tolist())) + [int(score.max()) + 1]:
        labels, clusters = labels_at(full, t)
        up = list(range(n))

        def find(v):
            while up[v] != v:
                v = up[v]
            return v
        for (i, j), s in zip(pairs.tolist(), score.tolist()):
            if s >= t:
                a, b = find(i), find(j)
                up[max(a, b)] = min(a, b)
        assert [find(v) for v in range(n)] == labels.tolist()
        assert clusters == n - int((score >= t).sum())
