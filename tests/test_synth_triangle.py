"""The reference machinery of tests/test_gpu_packed_index_64.py (tests/synth_triangle.py), checked on the CPU at sizes where
brute force is possible -- N = 2, 65, 300, through the code paths the big case takes (torch on the CPU, slices of a few
thousand elements so that there are many) -- and the index facts of N = 92 810."""
import numpy as np
import pytest
import torch

from tests import synth_triangle as st
from tests.linkage_ref import kruskal_tree, prim_tree
from tests.test_gpu_neighbors import expected_neighbors

SIZES = (2, 65, 300)
LIMIT = 4096     # elements per slice here: 11 slices at N = 300, and columns longer than... none; a slice is whole columns


def brute_full(n):
    """the symmetric matrix from value_int, pair by pair, Python integers; diagonal 0"""
    full = np.zeros((n, n), np.int64)
    for j in range(n):
        for i in range(j):
            full[i, j] = full[j, i] = st.value_int(i, j)
    return full


_full = {}


def full_of(n):
    if n not in _full:
        _full[n] = brute_full(n)
        _full[n].setflags(write=False)
    return _full[n]


def packed_of(full):
    n = full.shape[0]
    return np.concatenate([full[:j, j] for j in range(1, n)]) if n > 1 else np.zeros(0, np.int64)


def test_index_facts_of_the_big_case():
    n, p = st.N_BIG, st.P_BIG
    assert p == n * (n - 1) // 2 == 4306801645 and p > 2**32
    assert st.tri(65536) == 2147450880 and st.unpack(2**31) == (32768, 65536) and st.unpack(2**31 - 1) == (32767, 65536)
    assert st.tri(92682) == 4294930221 and st.unpack(2**32) == (37075, 92682) and st.unpack(2**32 - 1) == (37074, 92682)
    assert st.tri(92683) == 4295022903 and st.unpack(p - 1) == (n - 2, n - 1)
    beyond = [j for j in range(1, n) if st.tri(j) >= 2**32]
    assert beyond == list(range(92683, 92810)) and len(beyond) == 127
    blocks = sorted({j // 64 for j in beyond})
    whole = [b for b in blocks if all(st.tri(j) >= 2**32 and j < n for j in range(64 * b, 64 * b + 64))]
    assert whole == [92736 // 64] and (n - 1) // 64 == 92800 // 64 and n % 64 != 0   # one full block, then a partial last one
    # the slices of the big case: whole columns, in order, none above 2^27 elements, the triangle exactly
    cuts = list(st.column_slices(n))
    assert cuts[0][0] == 1 and cuts[-1][1] == n and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    assert max(st.tri(j1) - st.tri(j0) for j0, j1 in cuts) <= st.SLICE and len(cuts) < 40


def test_numpy_torch_and_python_integers_agree():
    rng = np.random.default_rng(5)
    j = rng.integers(1, st.N_BIG, 4000)
    i = rng.integers(0, j)
    i[:1000] = st.parent(j[:1000].astype(np.int64))      # planted ones among them
    a = st.value(i.astype(np.int64), j.astype(np.int64))
    b = st.value(torch.from_numpy(i), torch.from_numpy(j)).numpy()
    c = [st.value_int(int(x), int(y)) for x, y in zip(i, j)]
    assert a.dtype == np.int64 and np.array_equal(a, b) and a.tolist() == c
    assert (a[:1000] >= st.PLANT).all() and a.min() >= -2**31 and a.max() <= 2**31 - 1
    planted = a >= st.PLANT
    assert np.array_equal(planted, i == st.parent(j.astype(np.int64)))       # noise stays below every planted value
    # one row of the big case keeps the radix rounds of a byte-wise select busy: many distinct top bytes
    row = st.row_block(70000, 70001, st.N_BIG)[0].numpy()
    row = np.delete(row, 70000)
    assert len(np.unique(row)) > 92000 and len(np.unique((row + 2**31) >> 24)) >= 190
    # every weight occurs, each tied thousands of times, INT32_MAX among the values
    w = st.weight(np.arange(1, st.N_BIG, dtype=np.int64))
    assert sorted(np.unique(w).tolist()) == sorted(st.WEIGHTS) and np.bincount(np.searchsorted(sorted(st.WEIGHTS), w)).min() > 17000
    assert st.PLANT + max(st.WEIGHTS) == 2**31 - 1


@pytest.mark.parametrize("n", SIZES)
def test_fill_equals_value_pair_by_pair(n):
    full = full_of(n)
    packed = torch.full((st.tri(n) + 1,), -7, dtype=torch.int32)
    st.fill(packed, n, LIMIT)
    assert packed[-1] == -7
    assert np.array_equal(packed[:-1].numpy().astype(np.int64), packed_of(full))
    if n == 300:
        cuts = list(st.column_slices(n, LIMIT))
        assert len(cuts) > 10 and max(st.tri(b) - st.tri(a) for a, b in cuts) <= LIMIT
    # ... and the rows of the symmetric matrix, built without a packed index
    for r0 in range(0, n, 64):
        block = st.row_block(r0, min(r0 + 64, n), n).numpy()
        want = full[r0:r0 + 64].copy()
        want[np.arange(len(want)), np.arange(r0, r0 + len(want))] = st.DIAGONAL
        assert np.array_equal(block, want)


@pytest.mark.parametrize("n", SIZES)
def test_planted_tree_is_the_maximum_spanning_tree(n):
    full = full_of(n)
    pairs, score = st.planted_tree(n)
    for name, ref in (("prim", prim_tree), ("kruskal", kruskal_tree)):
        if name == "kruskal" and n > 65:
            continue
        want_pairs, want_score = ref(full)
        assert np.array_equal(pairs, want_pairs) and np.array_equal(score, want_score), (name, n)
    assert (score >= st.PLANT).all() and (np.sort(packed_of(full))[::-1][:n - 1] >= st.PLANT).all()


@pytest.mark.parametrize("n", SIZES)
def test_topk_keys_equal_the_lexsort(n):
    full = full_of(n)
    for k in sorted({1, min(5, n - 1), min(64, n - 1)}):
        want = expected_neighbors(full, k)
        index = np.concatenate([st.topk_rows(st.row_block(r0, min(r0 + 48, n), n), k)[0].numpy() for r0 in range(0, n, 48)])
        score = np.concatenate([st.topk_rows(st.row_block(r0, min(r0 + 48, n), n), k)[1].numpy() for r0 in range(0, n, 48)])
        assert np.array_equal(index, want[0]) and np.array_equal(score, want[1]), (n, k)
    # ties decide: a row of equal scores comes out by column, and INT32_MIN does not overflow the key
    block = torch.full((2, 70), -2**31, dtype=torch.int64)
    block[1, 40:] = 2**31 - 1
    index, score = st.topk_rows(block, 64)
    assert index[0].tolist() == list(range(64)) and index[1].tolist() == list(range(40, 70)) + list(range(34))
    assert score[1].tolist() == [2**31 - 1] * 30 + [-2**31] * 34


@pytest.mark.parametrize("n", SIZES)
def test_histogram_select_equals_sort(n):
    tri_sorted = np.sort(packed_of(full_of(n)))
    p = len(tri_sorted)
    ranks = sorted({0, p - 1, p // 2, p // 3, (p * 99) // 100, min(7, p - 1)})
    value, below = st.histogram_select(lambda: (v for *_, v in st.slice_values(n, limit=LIMIT)), ranks)
    assert value.tolist() == tri_sorted[ranks].tolist()
    assert below.tolist() == [int(np.searchsorted(tri_sorted, tri_sorted[k], side="left")) for k in ranks]


def test_histogram_select_with_ties_and_the_extremes():
    rng = np.random.default_rng(9)
    data = np.concatenate([rng.integers(-5, 5, 3000), [-2**31] * 7, [2**31 - 1] * 5, rng.integers(-2**31, 2**31, 2000)]).astype(np.int64)
    rng.shuffle(data)
    ordered = np.sort(data)
    ranks = [0, 6, 7, len(data) - 1, len(data) - 5, len(data) - 6, 2500, 2501, 1234]
    value, below = st.histogram_select(lambda: iter(torch.from_numpy(data).split(700)), ranks)
    assert value.tolist() == ordered[ranks].tolist()
    assert below.tolist() == [int(np.searchsorted(ordered, ordered[k], side="left")) for k in ranks]
    one = torch.full((5000,), 77, dtype=torch.int64)
    value, below = st.histogram_select(lambda: iter(one.split(999)), [0, 4999, 2500])
    assert value.tolist() == [77] * 3 and below.tolist() == [0] * 3


def test_normalized_equals_pythons_floor_division():
    n = 300
    den = st.denominators(n).astype(np.int64)
    big = st.denominators(st.N_BIG)
    assert (big > 0).mean() > 0.95 and (big == 0).sum() > 900 and (big < 0).sum() > 900
    assert (den == 0).sum() >= 3 and (den < 0).sum() >= 2
    full = full_of(n)
    for j0, j1, i, j, v in st.slice_values(n, limit=LIMIT):
        for rule in (0, 1, 2):
            got = st.normalized(v, torch.from_numpy(den)[i], torch.from_numpy(den)[j], rule).tolist()
            for x, a, b in zip(got[::37], i.tolist()[::37], j.tolist()[::37]):
                d = (min(den[a], den[b]), max(den[a], den[b]), den[a] + den[b])[rule]
                s = int(full[a, b]) * (2 if rule == 2 else 1) * 1000000
                want = -2**31 if d <= 0 else max(-2**31, min(2**31 - 1, s // int(d)))
                assert x == want, (rule, a, b)
    # saturation and the sign of the rounding, element by element
    s = torch.tensor([2**31 - 1, -2**31, -7, 7, -7, 5], dtype=torch.int64)
    d = torch.tensor([1, 1, 2000000, 2000000, -3, 0], dtype=torch.int64)
    assert st.normalized(s, d, d, 0).tolist() == [2**31 - 1, -2**31, -4, 3, -2**31, -2**31]
