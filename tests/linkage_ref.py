"""The expectation of the single-linkage tests, independent of the code under test (include/seqalign_hip.h: sa_ctx_linkage).

Pair i < j has packed index p = j (j - 1) / 2 + i; pair e comes before pair f iff score(e) > score(f), or the scores are equal
and p(e) < p(f).  The tree is the maximum spanning tree of the complete graph under that strict order, its N - 1 pairs sorted by
it.  prim_tree is Prim in NumPy over a full symmetric matrix with one int64 key per pair (valid for N <= 65 536: p < 2^32);
kruskal_tree is the definition in plain Python for small N; labels_at floods the boolean matrix of the entries at or above a threshold from the smallest unlabelled index."""
import numpy as np


def packed_index(i, j):
    lo, hi = np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)
    return hi * (hi - 1) // 2 + lo


def _sorted(lo, hi, score):
    lo, hi, score = np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(score, np.int64)
    order = np.lexsort((packed_index(lo, hi), -score))
    pairs = np.stack([lo[order], hi[order]], axis=1).astype(np.int32).reshape(-1, 2)
    return pairs, score[order].astype(np.int32)


def prim_tree(full: np.ndarray):
    """(pairs int32 (N - 1, 2), score int32 (N - 1,)) of a full symmetric matrix; the diagonal is never read as a pair"""
    n = full.shape[0]
    assert full.shape == (n, n) and 1 <= n <= 65536
    if n == 1:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    idx = np.arange(n, dtype=np.int64)
    none = np.iinfo(np.int64).min
    key = np.full(n, none, np.int64)   # the best pair from v into the tree: a larger key comes first
    other = np.zeros(n, np.int64)      # ... and its end inside the tree
    inside = np.zeros(n, bool)
    inside[0] = True
    last = 0
    lo, hi, score = [], [], []
    for _ in range(n - 1):
        k = (full[last].astype(np.int64) << 32) | (0xFFFFFFFF - packed_index(idx, np.where(idx == last, last + 1, last)))
        better = ~inside & (k > key)
        key[better] = k[better]
        other[better] = last
        pick = int(np.argmax(np.where(inside, none, key)))
        lo.append(min(pick, int(other[pick])))
        hi.append(max(pick, int(other[pick])))
        score.append(int(full[pick, other[pick]]))
        inside[pick] = True
        last = pick
    return _sorted(lo, hi, score)


def kruskal_tree(full: np.ndarray):
    """the definition: every pair in the contract's order, a pair joins iff its ends are in different components"""
    n = full.shape[0]
    pairs = sorted(((-int(full[i, j]), j * (j - 1) // 2 + i, i, j) for j in range(n) for i in range(j)))
    up = list(range(n))

    def find(v):
        while up[v] != v:
            up[v] = up[up[v]]
            v = up[v]
        return v
    lo, hi, score = [], [], []
    for neg, _, i, j in pairs:
        a, b = find(i), find(j)
        if a != b:
            up[max(a, b)] = min(a, b)
            lo.append(i)
            hi.append(j)
            score.append(-neg)
    return _sorted(lo, hi, score)


def _flood(a: np.ndarray):
    """labels of the components of a boolean adjacency matrix: flood from the smallest index that has no label yet, a whole
    frontier per step (every row is read once: N^2 bytes in all, where a Python loop over the entries of `a` would take
    seconds at N = 2 000)"""
    n = a.shape[0]
    labels = np.full(n, -1, np.int32)
    clusters = 0
    for r in range(n):
        if labels[r] >= 0:
            continue
        clusters += 1
        reach = np.zeros(n, bool)
        reach[r] = True
        frontier = np.array([r])
        while frontier.size:
            new = a[frontier].any(axis=0) & ~reach
            reach |= new
            frontier = np.flatnonzero(new)
        labels[reach] = r
    return labels, clusters


def labels_at(full: np.ndarray, t: int):
    """(labels int32 (N,), clusters): labels[r] = the smallest index in r's component of the graph full >= t (off the diagonal)"""
    a = full >= t
    np.fill_diagonal(a, False)
    return _flood(a)


def labels_from_csr(offsets: np.ndarray, index: np.ndarray):
    """labels of the components of a symmetric adjacency in CSR form (what hip_edges returns)"""
    n = offsets.size - 1
    a = np.zeros((n, n), bool)
    a[np.repeat(np.arange(n), np.diff(offsets)), index] = True
    return _flood(a)[0]


def random_full(n: int, spread: int, seed: int) -> np.ndarray:
    """a symmetric int32 matrix whose off-diagonal entries take `spread` distinct values (1: all equal)"""
    rng = np.random.default_rng(seed)
    m = np.triu(rng.integers(0, spread, size=(n, n)).astype(np.int32) - spread // 2, 1)
    return m + m.T


def packed_from(full: np.ndarray) -> np.ndarray:
    n = full.shape[0]
    return np.concatenate([full[:j, j] for j in range(1, n)]).astype(np.int32) if n > 1 else np.zeros(0, np.int32)
