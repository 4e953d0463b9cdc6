"""Deterministic EXTREMAL inputs: sequences that drive the DP values of a scoring to the top and to the bottom of what
the kernels' value-range bounds (sequencealigner_amd/csrc/sa_limits.cpp) allow -- a perfect diagonal of the
best-scoring residue over every column of a class, the matrix minimum in every cell, one long gap, and runs of the
shortest sequences behind every long one (as many frame shifts in flight as the lane group can hold).

Everything is derived from a Scoring's `lut` and `sub` (no letters are hard-coded: protein and nucleotide matrices
alike) and from the class geometry below.  Pure numpy; used by tests/test_gpu_value_range.py and tools/gpu_fuzz.py."""
from __future__ import annotations

import numpy as np

SUB_DIM = 24
# column budgets W of the packed classes (sa_shapes.h): 8-lane groups K = 1..24, 16-lane groups K = 13..64
CLASS_WIDTHS = [8 * k for k in range(1, 25)] + [16 * k for k in range(13, 65)]
MAX_PACKED_LEN = 1024
SHORTEST = (1, 2, 3, 7, 15)
PK_WPB = 4  # SA_PK_WPB: waves of a packed workgroup (eight for the widest classes)


def letters(scoring) -> list[int]:
    """the upper-case letters the scoring's matrix knows, in alphabetical order"""
    return [c for c in range(ord("A"), ord("Z") + 1) if scoring.lut[c] >= 0]


def _score(scoring, a: int, b: int) -> int:
    return int(scoring.sub[SUB_DIM * int(scoring.lut[a]) + int(scoring.lut[b])])


def best_residue(scoring) -> bytes:
    """the residue with the largest diagonal entry (the first in the alphabet among equals)"""
    ls = letters(scoring)
    return bytes([max(ls, key=lambda c: (_score(scoring, c, c), -c))])


def worst_pair(scoring) -> tuple[bytes, bytes]:
    """(b, c): a pair of residues that attains the minimum of the matrix over its letters"""
    ls = letters(scoring)
    lo, b, c = min((_score(scoring, x, y), x, y) for x in ls for y in ls)
    return bytes([b]), bytes([c])


def ladder(limit: int = MAX_PACKED_LEN) -> list[int]:
    """W - 1, W, W + 1 for every class width, ascending, nothing above `limit`"""
    return sorted({n for w in CLASS_WIDTHS for n in (w - 1, w, w + 1) if 1 <= n <= limit})


def class_lengths(widths, limit: int = MAX_PACKED_LEN) -> list[int]:
    """the part of the ladder around the given class widths"""
    return sorted({n for w in widths for n in (w - 1, w, w + 1) if 1 <= n <= limit})


def top_store(scoring, lengths=None) -> list[bytes]:
    """homopolymers of the best residue at every ladder length, the ascending ladder twice: every length is a column
    (the later sequence of a pair) behind every other length and a row in front of it -- each pair of the second copy
    with its twin in the first is a perfect diagonal over all W columns"""
    best = best_residue(scoring)
    lengths = ladder() if lengths is None else list(lengths)
    return [best * n for n in lengths] * 2


def block_pair(scoring, n: int) -> tuple[bytes, bytes]:
    """best^n b^n against c^n best^n: the best alignment pairs the two best^n halves and opens one long gap on each
    side of them"""
    best = best_residue(scoring)
    b, c = worst_pair(scoring)
    return best * n + b * n, c * n + best * n


def bottom_store(scoring, lengths=None, blocks=(4, 20, 96, 250, 512)) -> list[bytes]:
    """homopolymers of b (rows, first) against homopolymers of c (columns, behind them): the matrix minimum in every
    cell; then the block sequences x = best^n b^n, y = c^n best^n as x, y, x -- y a column against x and a row in
    front of it -- whose alignments live on Gotoh's gap registers and on SW's floor"""
    b, c = worst_pair(scoring)
    lengths = ladder() if lengths is None else list(lengths)
    seqs = [b * n for n in lengths] + [c * n for n in lengths]
    for n in blocks:
        x, y = block_pair(scoring, n)
        seqs += [x, y, x]
    return seqs


def frame_run(m: int) -> int:
    """2 live + 2 with live of the 16-lane groups: the last rows of a sequence travel through 15 more lanes while a
    terminator enters every m + 1 steps"""
    return 2 * (1 + 15 // (m + 1)) + 2


def frames_store(scoring, m: int, lengths=None, run: int | None = None, blocks=(4, 20, 96)) -> list[bytes]:
    """the top and bottom stores with a run of `run` shortest sequences (lengths m, m + 1, m, ...) in store order directly
    behind every long one: behind a top sequence they are made of the best residue, behind a bottom sequence of b (block
    sequences no longer than the shortest ones are left out: m stays the store's minimum)"""
    best = best_residue(scoring)
    b, _ = worst_pair(scoring)
    run = frame_run(m) if run is None else run
    blocks = [n for n in blocks if 2 * n > m + 1]
    out = []
    for letter, seqs in ((best, top_store(scoring, lengths)), (b, bottom_store(scoring, lengths, blocks))):
        shorts = [letter * (m + (k & 1)) for k in range(run)]
        for s in seqs:
            out.append(s)
            out += shorts
    return out


def full_stream_store(scoring, length: int, chunk: int, columns=(), seed: int = 0) -> list[bytes]:
    """rows for a whole tile of maximal streams: PK_WPB x 8 x chunk sequences of the longest length -- a full tile streams
    `chunk` of them per lane group, whatever the group width.  Of every eight rows four in a row are homopolymers of the
    best residue (with chunk = 4 a whole stream: the largest drift under the largest score), then b, c and two uniform
    random ones.  Behind them the columns: best, c and a random sequence of that length, and best and c homopolymers of
    every length in `columns`."""
    best = best_residue(scoring)
    b, c = worst_pair(scoring)
    ls = np.array(letters(scoring), np.uint8)
    rng = np.random.default_rng(seed)
    seqs = []
    for k in range(PK_WPB * 8 * chunk):
        seqs.append(best * length if k % 8 < 4 else b * length if k % 8 == 4 else c * length if k % 8 == 5
                    else ls[rng.integers(0, ls.size, length)].tobytes())
    seqs += [best * length, c * length, ls[rng.integers(0, ls.size, length)].tobytes()]
    for n in columns:
        seqs += [best * n, c * n]
    return seqs


def low_complexity(scoring, rng, n: int, m: int, long_lo: int = 40, long_hi: int = MAX_PACKED_LEN) -> list[bytes]:
    """fuzzer regime: homopolymers and two-letter sequences over {best, b, c}, the shortest of length m"""
    best = best_residue(scoring)
    b, c = worst_pair(scoring)
    seqs = []
    for _ in range(n):
        x, y = [(best, best), (b, b), (c, c), (best, b), (c, best), (b, c)][int(rng.integers(0, 6))]
        ln = m + int(rng.integers(0, 2)) if rng.random() < 0.5 else int(rng.integers(long_lo, long_hi + 1))
        kind = int(rng.integers(0, 3))
        if kind == 0 or ln < 2:
            s = x * ln
        elif kind == 1:  # two blocks
            cut = int(rng.integers(1, ln))
            s = x * cut + y * (ln - cut)
        else:  # a short period
            p = int(rng.integers(1, 5))
            s = ((x * p + y * p) * (ln // (2 * p) + 1))[:ln]
        seqs.append(s)
    seqs[int(rng.integers(0, n))] = best * m  # the shortest length really occurs
    return seqs
