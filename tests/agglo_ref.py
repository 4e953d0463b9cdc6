"""The expectation of the complete- and average-linkage tests, independent of the code under test (include/seqalign_hip.h:
sa_ctx_agglomerate).

A cluster is named by its smallest member.  The similarity of two clusters is the minimum score over their cross pairs
(complete) or the exact rational S / (|A| |B|), S the sum of those scores (average).  Cluster pair (A, B) with names a < b has
p = b (b - 1) / 2 + a; a pair comes before another iff its similarity is larger, or equal with the smaller p.  Every step merges
the first pair among the active clusters; the union keeps the name a.  score is the minimum, or the floor of the average.

agglo_fractions is that definition in plain Python with fractions.Fraction, for N <= 40.  agglo_numpy is the same greedy over a
matrix that shrinks with every merge, for N <= 700: complete linkage in integers; average linkage by a float candidate that is
then settled by exact int64 cross-multiplication -- valid while |S| n < 2^62, which the function asserts.  merge_table turns
the pairs into scipy's convention through a plain union-find."""
from fractions import Fraction

import numpy as np

COMPLETE, AVERAGE = 1, 2
METHODS = {"complete": COMPLETE, "average": AVERAGE}


def _result(pairs, score):
    return np.array(pairs, np.int32).reshape(-1, 2), np.array(score, np.int32)


def agglo_fractions(full: np.ndarray, method: int):
    """(pairs int32 (N - 1, 2), score int32 (N - 1,)) by the definition; every step looks at every pair of clusters"""
    n = full.shape[0]
    assert full.shape == (n, n) and 1 <= n <= 40 and method in (COMPLETE, AVERAGE)
    members = {v: [v] for v in range(n)}
    pairs, score = [], []
    for _ in range(n - 1):
        first = None
        for b in sorted(members):
            for a in sorted(members):
                if a >= b:
                    continue
                cross = [int(full[x, y]) for x in members[a] for y in members[b]]
                sim = Fraction(min(cross)) if method == COMPLETE else Fraction(sum(cross), len(cross))
                key = (-sim, b * (b - 1) // 2 + a)
                if first is None or key < first[0]:
                    first = (key, a, b, sim)
        _, a, b, sim = first
        pairs.append((a, b))
        score.append(sim.numerator // sim.denominator)  # (floor: Python's //)
        members[a] += members.pop(b)
    return _result(pairs, score)


def agglo_numpy(full: np.ndarray, method: int, stats: dict | None = None):
    """the same tree for N <= 700.  stats (average linkage): 'closest' = over all steps, the smallest relative distance
    |x - y| / |x| of a runner-up y to the winner x as an exact Fraction (0: an exact tie of two different cluster pairs);
    'mixed_ties' = the steps whose first pairs tie as the same rational in different terms (S, n)"""
    n = full.shape[0]
    assert full.shape == (n, n) and 1 <= n <= 700 and method in (COMPLETE, AVERAGE)
    names = np.arange(n, dtype=np.int64)
    size = np.ones(n, np.int64)
    w = full.astype(np.int64)  # minima or sums
    upper_all = np.triu(np.ones((n, n), bool), 1)
    pairs, score = [], []
    closest = None
    for _ in range(n - 1):
        k = names.size
        upper = upper_all[:k, :k]  # (names ascend: position i < j is name i < name j)
        if method == COMPLETE:
            top = w[upper].max()
            ties = (w == top) & upper
            value = int(top)
        else:
            nn = np.outer(size, size)
            assert int(np.abs(w).max()) * int(nn.max()) < 2**62, "the exact comparison needs |S| n < 2^62"
            approx = np.where(upper, w / nn, -np.inf)
            i, j = np.unravel_index(int(np.argmax(approx)), approx.shape)
            for _ in range(k * k):  # (each round moves to a strictly larger rational)
                s0, n0 = int(w[i, j]), int(nn[i, j])
                ahead = w * n0 - s0 * nn  # > 0: that pair's average is above the candidate's, exactly
                above = (ahead > 0) & upper
                if not above.any():
                    break
                i, j = np.unravel_index(int(np.argmax(np.where(above, approx, -np.inf))), approx.shape)
            ties = (ahead == 0) & upper
            value = s0 // n0
            if stats is not None and np.unique(nn[ties]).size > 1:  # the same rational in different terms (S, n)
                stats["mixed_ties"] = stats.get("mixed_ties", 0) + 1
            if stats is not None and k > 2:
                other = upper.copy()
                other[i, j] = False
                near = int(np.argmin(np.abs(ahead[other]) / nn[other].astype(np.float64)))  # (|x - y| = |ahead| / (n0 n))
                s1, n1 = int(w[other][near]), int(nn[other][near])
                if s0:
                    rel = abs(Fraction(s0, n0) - Fraction(s1, n1)) / abs(Fraction(s0, n0))
                    closest = rel if closest is None else min(closest, rel)
        ti, tj = np.nonzero(ties)
        p = names[tj] * (names[tj] - 1) // 2 + names[ti]
        at = int(np.argmin(p))
        i, j = int(ti[at]), int(tj[at])
        pairs.append((int(names[i]), int(names[j])))
        score.append(value)
        merged = np.minimum(w[i], w[j]) if method == COMPLETE else w[i] + w[j]
        w[i, :] = merged
        w[:, i] = merged
        size[i] += size[j]
        keep = np.arange(k) != j
        w = w[keep][:, keep]
        names, size = names[keep], size[keep]
    if stats is not None:
        stats["closest"] = closest
    return _result(pairs, score)


def merge_table(pairs: np.ndarray, n: int) -> np.ndarray:
    """int32 (N - 1, 3): rows (left, right, size) in the convention of scipy.cluster.hierarchy -- ids below N are sequences,
    id N + u is the cluster made by merge u -- through a plain union-find"""
    up, ident, members = list(range(n)), list(range(n)), [1] * n

    def find(v):
        while up[v] != v:
            v = up[v]
        return v
    out = []
    for t, (lo, hi) in enumerate(np.asarray(pairs).tolist()):
        a, b = find(lo), find(hi)
        assert a != b
        out.append((min(ident[a], ident[b]), max(ident[a], ident[b]), members[a] + members[b]))
        root, other = min(a, b), max(a, b)
        up[other] = root
        ident[root] = n + t
        members[root] = out[-1][2]
    return np.array(out, np.int32).reshape(-1, 3)


def labels_of(pairs: np.ndarray, score: np.ndarray, n: int, t: int):
    """(labels int32 (N,), clusters) after the merges with score >= t (a prefix): labels[r] = the smallest index in r's cluster"""
    labels = np.arange(n, dtype=np.int32)
    clusters = n
    for (lo, hi), s in zip(np.asarray(pairs).tolist(), np.asarray(score).tolist()):
        if s < t:
            break
        a, b = int(labels[lo]), int(labels[hi])
        labels[labels == max(a, b)] = min(a, b)
        clusters -= 1
    return labels, clusters


def tie_free_full(n: int, seed: int) -> np.ndarray:
    """a symmetric int32 matrix whose N (N - 1) / 2 pairs hold distinct values: a random permutation, spread out so that
    averages of different groups do not meet either"""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n, 1)
    full = np.zeros((n, n), np.int32)
    full[i, j] = full[j, i] = (rng.permutation(i.size) * 7 - 3 * i.size).astype(np.int32)
    return full
