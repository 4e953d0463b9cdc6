"""A packed triangle in closed form, for the tests of packed indices at and beyond 2^32 (tests/test_gpu_packed_index_64.py;
tests/test_synth_triangle.py checks this module itself where brute force is possible).

value(i, j), i < j, is a function of the pair alone.  The expectations of the tests are computed from it through (i, j) --
row_block, planted_tree, histogram_select, normalized -- and never through the packed index j (j - 1) / 2 + i that the kernels
under test compute; only fill, which lays the matrix out for them, uses that index, in Python and torch int64.

The values:
  noise    mix(seed(i, j)) mod 3 * 2^30 - 2^31, seed = (i * 2654435761 + j * 40503 + (i ^ j) * 97) mod 2^32: every value of
           [-2^31, 2^30) occurs (the lowest 2^30 twice as often as the others), INT32_MIN included
  planted  for j >= 1 the entry (parent(j), j), parent(j) = mix(j ^ PARENT_SALT) mod j, is 2^30 + weight(j), weight(j) one of
           WEIGHTS by mix(j ^ WEIGHT_SALT) mod 5: above every noise value, INT32_MAX among them, every weight tied about N / 5
           times.  The N - 1 planted pairs are a spanning tree (parent(j) < j) and each beats every pair that is not planted, so
           the maximum spanning tree is the planted tree under any tie rule; the contract's order (include/seqalign_hip.h:
           higher score first, then smaller packed index) only sorts it.

All arithmetic is int64 on values masked to 32 bits before every multiplication, multipliers of the mix below 2^30 (products
below 2^62; the seed's i * 2654435761 stays below 2^49 for i < 2^17): the same bits from NumPy, from torch on the CPU and on a
device, and from Python's integers (value_int).  An array argument decides the library: NumPy arrays in, NumPy out; torch
tensors in, torch out on their device."""
import numpy as np

N_BIG = 92810
MASK = 0xFFFFFFFF
PLANT = 2**30
WEIGHTS = (0, 1, 2, 3, 2**30 - 1)
PARENT_SALT, WEIGHT_SALT = 0x2545F491, 0x1B873593
DIAGONAL = -2**40      # row_block's diagonal: below every int32, so never a neighbour, never an edge
KEY_SHIFT = 2**20      # top-k key = score * 2^20 - column: one int64 per candidate, no overflow for any int32 score (|key| < 2^52)
SLICE = 2**27          # fill / column_slices: at most this many elements at a time


def tri(j: int) -> int:
    return j * (j - 1) // 2


def unpack(p: int):
    """(i, j) of packed index p, Python integers"""
    import math
    j = (1 + math.isqrt(1 + 8 * p)) // 2
    assert tri(j) <= p < tri(j + 1)
    return p - tri(j), j


# the facts the big case rests on (Python integers)
P_BIG = tri(N_BIG)
assert P_BIG == 4306801645 > 2**32
assert tri(65536) == 2147450880 and unpack(2**31) == (32768, 65536)
assert tri(92682) == 4294930221 and unpack(2**32) == (37075, 92682)
assert tri(92683) == 4295022903 > 2**32 and unpack(2**32 - 1)[1] == 92682
assert N_BIG - 92683 == 127 and 92736 % 64 == 0 and 92683 < 92736 and 92736 + 64 == 92800 < N_BIG   # one full block of 64 columns beyond 2^32
assert N_BIG < 2**17 and KEY_SHIFT > N_BIG


def _where(cond, a, b):
    if isinstance(cond, np.ndarray):
        return np.where(cond, a, b)
    import torch
    return torch.where(cond, a, b)


def mix(x):
    """three multiply-xorshift rounds on 32-bit values held in int64 (or Python integers)"""
    x = x & MASK
    x = ((x ^ (x >> 16)) * 0x2C1B3C6D) & MASK
    x = ((x ^ (x >> 12)) * 0x297A2D39) & MASK
    x = ((x ^ (x >> 15)) * 0x3243F6A9) & MASK
    return x ^ (x >> 16)


def parent(j):
    """j >= 1 (an array may hold 0: its parent is then 0 and never used)"""
    if isinstance(j, int):
        return mix(j ^ PARENT_SALT) % j
    return mix(j ^ PARENT_SALT) % _where(j > 0, j, j + 1)


def weight(j):
    w = mix(j ^ WEIGHT_SALT) % 5
    if isinstance(j, int):
        return WEIGHTS[w]
    return w + (w == 4) * (WEIGHTS[4] - 4)


def noise(i, j):
    seed = (i * 2654435761 + j * 40503 + (i ^ j) * 97) & MASK
    return mix(seed) % (3 * 2**30) - 2**31


def value(i, j):
    """int64 arrays (NumPy or torch) of pairs i < j, element by element"""
    return _where(i == parent(j), PLANT + weight(j), noise(i, j))


def value_int(i: int, j: int) -> int:
    assert 0 <= i < j
    return PLANT + weight(j) if i == parent(j) else noise(i, j)


def column_slices(n: int, limit: int = SLICE):
    """column ranges [j0, j1), 1 <= j0 < j1 <= n, that cover the triangle in order, each of at most `limit` elements (one column
    where a column alone is longer)"""
    j0 = 1
    while j0 < n:
        j1 = j0 + 1
        while j1 < n and tri(j1 + 1) - tri(j0) <= limit:
            j1 += 1
        yield j0, j1
        j0 = j1


def slice_pairs(j0: int, j1: int, device="cpu"):
    """(i, j) of the pairs of columns [j0, j1) in packed order, torch int64: column after column, i ascending within"""
    import torch
    cols = torch.arange(j0, j1, dtype=torch.int64, device=device)
    j = torch.repeat_interleave(cols, cols)
    first = torch.cumsum(cols, 0) - cols                       # where each column begins within the slice
    i = torch.arange(j.numel(), dtype=torch.int64, device=device) - torch.repeat_interleave(first, cols)
    return i, j


def slice_values(n: int, device="cpu", limit: int = SLICE):
    """yields (j0, j1, i, j, value(i, j)) over column_slices(n): the whole triangle from the closed form, (i, j) from the column
    ranges"""
    for j0, j1 in column_slices(n, limit):
        i, j = slice_pairs(j0, j1, device)
        yield j0, j1, i, j, value(i, j)


def fill(packed, n: int, limit: int = SLICE) -> None:
    """packed[tri(j) + i] = value(i, j) for a torch int32 tensor of at least tri(n) elements, slice by slice on its device"""
    import torch
    assert packed.dtype == torch.int32 and packed.numel() >= tri(n)
    for j0, j1, _, _, v in slice_values(n, packed.device, limit):
        packed[tri(j0):tri(j1)] = v.to(torch.int32)


def row_block(r0: int, r1: int, n: int, device="cpu"):
    """rows [r0, r1) of the symmetric matrix, torch int64 (r1 - r0, n): value(min(r, c), max(r, c)), DIAGONAL at c == r"""
    import torch
    r = torch.arange(r0, r1, dtype=torch.int64, device=device)[:, None].expand(r1 - r0, n)
    c = torch.arange(n, dtype=torch.int64, device=device)[None, :].expand(r1 - r0, n)
    lo, hi = torch.minimum(r, c), torch.maximum(r, c)
    return torch.where(r == c, DIAGONAL, value(lo, hi))


def topk_rows(block, k: int):
    """(index, score), int32 (rows, k): per row of a row_block the k best columns, score descending then column ascending, by
    one unique int64 key per candidate"""
    import torch
    cols = torch.arange(block.shape[1], dtype=torch.int64, device=block.device)
    best = torch.topk(block * KEY_SHIFT - cols[None, :], k, dim=1, sorted=True).indices
    return best.to(torch.int32), torch.gather(block, 1, best).to(torch.int32)


def planted_tree(n: int):
    """(pairs int32 (n - 1, 2), score int32 (n - 1,)): the planted pairs in the contract's order -- higher score first, then
    smaller packed index -- NumPy int64"""
    j = np.arange(1, n, dtype=np.int64)
    lo, score = parent(j), PLANT + weight(j)
    order = np.lexsort((j * (j - 1) // 2 + lo, -score))
    return np.stack([lo[order], j[order]], axis=1).astype(np.int32).reshape(-1, 2), score[order].astype(np.int32)


def histogram_select(chunks, ranks):
    """(value, below) per rank of the multiset of int32 scores that `chunks()` yields as int64 torch tensors (called twice), by a
    two-level histogram of 16 bits each: bincount of the top half of score + 2^31 over all chunks, then, among the entries that
    share a rank's top half, bincount of the low half.  Counts are accumulated in int64 on the CPU.  below = entries < value."""
    import torch
    first = torch.zeros(65536, dtype=torch.int64)
    for v in chunks():
        first += torch.bincount((v + 2**31) >> 16, minlength=65536).cpu()
    total = int(first.sum())
    before = (torch.cumsum(first, 0) - first).tolist()          # entries whose top half is smaller
    first = first.tolist()
    tops = []
    for k in ranks:
        assert 0 <= k < total, (k, total)
        t = next(t for t in range(65535, -1, -1) if before[t] <= k and first[t])    # the last bin that begins at or below k
        assert before[t] <= k < before[t] + first[t]
        tops.append(t)
    second = {t: torch.zeros(65536, dtype=torch.int64) for t in set(tops)}
    for v in chunks():
        u = v + 2**31
        top = u >> 16
        for t in second:
            second[t] += torch.bincount(u[top == t] & 0xFFFF, minlength=65536).cpu()
    values, below = [], []
    for k, t in zip(ranks, tops):
        assert int(second[t].sum()) == first[t]
        inner = (torch.cumsum(second[t], 0) - second[t]).tolist()
        counts = second[t].tolist()
        low = next(b for b in range(65535, -1, -1) if inner[b] <= k - before[t] and counts[b])
        values.append((t << 16 | low) - 2**31)
        below.append(before[t] + inner[low])
    return np.array(values, np.int32), np.array(below, np.int64)


# ---- normalised scores (include/seqalign_hip.h: sa_ctx_normalize) -------------------------------------------------------------------
NORM_SCALE = 1000000
DEN_SALT = 0x68E31DA4


def denominators(n: int):
    """n int32 of a mix (NumPy): [2^28, 2^31) mostly, so that scores near 2^30 give ratios of a few parts per million up to a few
    million; every 97th is 0, every 101st negative"""
    k = np.arange(n, dtype=np.int64)
    d = 2**28 + mix(k ^ DEN_SALT) % (2**31 - 2**28)
    d = np.where(k % 101 == 5, -d, d)
    return np.where(k % 97 == 3, 0, d).astype(np.int32)


def normalized(s, di, dj, rule: int):
    """the value rule in torch int64, element by element: MIN 0, MAX 1, MEAN 2; floor division, D <= 0 gives INT32_MIN,
    saturated to int32"""
    import torch
    den = (torch.minimum(di, dj), torch.maximum(di, dj), di + dj)[rule]
    num = s * (2 * NORM_SCALE if rule == 2 else NORM_SCALE)
    q = torch.div(num, torch.clamp(den, min=1), rounding_mode="floor")
    return torch.where(den <= 0, -2**31, torch.clamp(q, -2**31, 2**31 - 1))
