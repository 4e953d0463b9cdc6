"""What the two-strand tests share (tests/test_gpu_strands.py, tests/test_gpu_strands_stream_order.py, tests/test_gpu_strands_cli.py,
tests/test_strands_host.py): the reverse complement written in Python, the inputs, and the expectation of a folded search, which
never comes from the code under test: fwd = oracle_rect(db, Q), rev = oracle_rect(db, rc(Q)), strand = rev > fwd,
best = where(strand, rev, fwd), hits = expected_hits(best, k) (tests/search_cases.py)."""
import numpy as np

from tests.search_cases import expected_hits, oracle_rect

ALPHABET = b"ATGCSWRYKMBVHDN*"
COMPLEMENT = dict(zip(b"ATGCSWRYKMBVHDN*U", b"TACGSWYRMKVBDHN*A"))
PALINDROMES = (b"ACGT" * 12, b"GAATTC" * 9)  # each is its own reverse complement


def rc(seq: bytes) -> bytes:
    return bytes(COMPLEMENT[c] for c in reversed(seq))


assert all(rc(p) == p for p in PALINDROMES)


def dna_database(n: int, seed: int, lo: int = 40, hi: int = 90) -> list:
    """random DNA, about one residue in twelve an IUPAC ambiguity code or '*'"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), ln)
        amb = rng.random(ln) < 1 / 12
        s[amb] = rng.choice(np.frombuffer(ALPHABET[4:], np.uint8), int(amb.sum()))
        out.append(s.tobytes())
    return out


def dna_queries(db_seqs, m: int, seed: int, lengths=None) -> list:
    """mutated substrings of database entries, every second one reverse-complemented first; with m >= 3 the last two queries are
    reverse-complement palindromes, whose two rows tie everywhere.  `lengths`: the queries' lengths instead (random DNA spliced
    around a mutated database entry, every second one reverse-complemented; no palindromes)"""
    rng = np.random.default_rng(seed)
    out = []
    plain = m if lengths is not None or m < 3 else m - 2
    for t in range(plain):
        src = bytearray(db_seqs[int(rng.integers(0, len(db_seqs)))])
        if lengths is None:
            a = int(rng.integers(0, max(len(src) - 30, 1)))
            src = src[a:a + int(rng.integers(24, 61))]
        for p in np.flatnonzero(rng.random(len(src)) < 0.08):
            src[p] = b"ACGT"[int(rng.integers(0, 4))]
        q = bytes(src)
        if lengths is not None:
            ln = int(lengths[t])
            filler = rng.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes()
            q = (q + filler)[:ln] if ln <= len(q) else filler[:(ln - len(q)) // 2] + q + filler[(ln - len(q)) // 2:ln - len(q)]
            assert len(q) == ln
        out.append(rc(q) if t % 2 else q)
    if plain < m:
        out += list(PALINDROMES)
    assert len(out) == m
    return out


class Folded:
    """the expectation of one case under one pair of value rectangles"""

    def __init__(self, fwd, rev, vfwd=None, vrev=None):
        self.fwd, self.rev = fwd, rev
        self.vfwd, self.vrev = (fwd, rev) if vfwd is None else (vfwd, vrev)
        self.strand = (self.vrev > self.vfwd)
        self.vbest = np.where(self.strand, self.vrev, self.vfwd).astype(np.int32)
        self.best = np.where(self.strand, rev, fwd).astype(np.int32)
        self.m, self.n = fwd.shape

    def bits(self) -> np.ndarray:
        """(M, words) uint64: bit d & 63 of word d >> 6"""
        words = (self.n + 63) // 64
        out = np.zeros((self.m, words), np.uint64)
        r, d = np.nonzero(self.strand)
        np.bitwise_or.at(out, (r, d >> 6), np.uint64(1) << (d & 63).astype(np.uint64))
        return out

    def hits(self, k: int):
        """(index, value, score, strand) of the k best by folded value"""
        index, value = expected_hits(self.vbest, k)
        at = index.astype(np.int64)
        return index, value, np.take_along_axis(self.best, at, 1), np.take_along_axis(self.strand, at, 1).astype(np.uint8)

    def above(self, min_value: int):
        """(offsets, index, value, score, strand) of the hits with folded value >= min_value, ascending d per row"""
        keep = self.vbest.astype(np.int64) >= int(min_value)
        offsets = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
        r, d = np.nonzero(keep)
        return offsets, d.astype(np.int32), self.vbest[r, d], self.best[r, d], self.strand[r, d].astype(np.uint8)


def folded_case(sa, oracle, db_seqs, query_seqs, scoring) -> Folded:
    fwd = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
    rev = oracle_rect(sa, oracle, db_seqs, [rc(q) for q in query_seqs], scoring)
    return Folded(fwd, rev)


def assert_not_degenerate(exp: Folded, k: int, palindromes: int, what: str) -> None:
    """conditions on the EXPECTED arrays, before the device is compared: both strands occur among the selected hits, at least one
    selected hit has fwd == rev (by value) and strand 0, the palindrome rows are all forward"""
    index, _, _, strand = exp.hits(k)
    at = index.astype(np.int64)
    assert (strand == 0).any() and (strand == 1).any(), f"{what}: one strand only among the selected hits"
    tie = np.take_along_axis(exp.vfwd, at, 1) == np.take_along_axis(exp.vrev, at, 1)
    assert (tie & (strand == 0)).any() and not (tie & (strand == 1)).any(), f"{what}: no selected hit ties between the strands"
    if palindromes:
        assert np.array_equal(exp.vfwd[-palindromes:], exp.vrev[-palindromes:]) and not exp.strand[-palindromes:].any(), f"{what}: palindrome rows"
