"""The store of tests/test_gpu_fit_strips.py and of the strip conditions in tests/test_fit_ref.py: plain Python, no device, no
library.  Four-letter DNA (A, C, G, T only: four letters tie everywhere), queries of three to five strips of 64 columns whose end lane
(n - 1) & 63 sits at 0, 1, 62 and 63, cut out of database entries with substitutions, inserted runs across the strip edges and
deletions, next to tandem repeats (plateaus in column n), and the conditions a reference over that store has to meet before a
device is compared with it -- counted here, from tests/fit_ref.py alone.

strip_store() -> (db, queries, notes); pairs(db, queries, notes) -> the 124 (query, database sequence) pairs; references(scoring, ...) the
three walks of every pair over one fill; counts(...) the conditions; check_floors what they must reach.

Cost of the Python reference: the 11 x 11 block is 2488 x 2309 = 5.7 M cells, each of the three pairs against the 3000-residue entry
about 1 M cells (3000 x 320, x 193, x 130: 1.9 M together), roughly a second of Python each; 7.7 M cells a scoring."""
from __future__ import annotations

import numpy as np

from tests import fit_ref
from tests.synth import make_dna_set

DB_RANDOM = (63, 64, 65, 130, 200, 257, 400, 700)
LONG = 3000
SEED = 3100
STRIP_EDGES = (64, 128, 192, 256)  # columns 64 | 65, 128 | 129, ...: lane 63 of a strip writes what lane 0 of the next one reads
# the cut-out queries: (database entry, start in it, length of the query, inserted runs (query position, length), deletions (query
# position, residues of the entry left out)); positions count from 0, so the run (60, 10) is columns 61 .. 70
CUTS = (
    (5, 40, 129, ((61, 6),), ((100, 6),)),
    (6, 50, 192, ((60, 10), (126, 5)), ((90, 5), (160, 7))),
    (6, 150, 193, ((62, 4), (125, 9)), ((150, 5),)),
    (7, 100, 257, ((60, 10), (127, 2), (188, 10)), ((100, 7), (220, 5))),
    (7, 330, 320, ((63, 2), (125, 9), (190, 6), (250, 9)), ((160, 6),)),
)
QUERY_LENGTHS = (129, 192, 193, 257, 320, 193, 256, 191, 255, 130, 193)
LONG_QUERIES = (4, 5, 9)  # against the 3000-residue entry: the 320, the repeat of 193 and the random 130


def dna(length: int, seed: int) -> bytes:
    return make_dna_set(1, length, length, seed)[0]


def cut_out(entry: bytes, start: int, length: int, inserts, deletions, seed: int) -> bytes:
    """entry[start ..) with about 5 % substitutions, random runs inserted at the query positions of `inserts`, residues of the entry
    left out at the query positions of `deletions`, `length` residues long; strictly inside the entry"""
    rng = np.random.default_rng(seed)
    events = sorted([(at, "I", ln) for at, ln in inserts] + [(at, "D", ln) for at, ln in deletions])
    out, src = bytearray(), start
    for at, kind, ln in events + [(length, "", 0)]:
        assert len(out) <= at, "the runs overlap"
        while len(out) < at:
            ch = entry[src]
            if rng.integers(20) == 0:
                ch = b"ACGT"[(b"ACGT".index(ch) + 1 + int(rng.integers(3))) % 4]  # another letter
            out.append(ch)
            src += 1
        if kind == "I":
            out += bytes(b"ACGT"[int(k)] for k in rng.integers(0, 4, ln))
        elif kind == "D":
            src += ln
    assert len(out) == length and 0 < start and src < len(entry), "the cut does not sit strictly inside"
    assert all(5 <= ln <= 7 for _, ln in deletions) and all(2 <= ln <= 10 for _, ln in inserts) and 1 <= len(deletions) <= 2
    assert all(any(at < edge and at + ln > edge for edge in STRIP_EDGES) for at, ln in inserts), "a run covers no strip edge"
    return bytes(out)


def strip_store():
    """(db, queries, notes): 12 database sequences, 11 queries; notes names the indices the tests speak of"""
    db = [dna(ln, SEED + ln) for ln in DB_RANDOM]
    db += [b"ACGT" * 60, (b"AC" * 40 + b"GGT") * 3, b"ACG" * 40, dna(LONG, SEED + LONG)]
    queries = [cut_out(db[d], start, ln, ins, dels, 70 + k) for k, (d, start, ln, ins, dels) in enumerate(CUTS)]
    queries += [b"ACGT" * 48 + b"A", b"AC" * 128, (b"AC" * 40 + b"GGT") * 2 + b"AC" * 12 + b"A"]
    queries += [dna(255, SEED + 1255), dna(130, SEED + 1130), b"T" * 193]
    assert [len(s) for s in db] == list(DB_RANDOM) + [240, 249, 120, LONG] and [len(s) for s in queries] == list(QUERY_LENGTHS)
    assert all(not set(s) - set(b"ACGT") for s in db + queries) and b"T" not in db[10]
    # the end lane (n - 1) & 63 at 0, 1, 62 and 63, in the third, fourth and fifth strip
    assert {(n - 1) & 63 for n in QUERY_LENGTHS} == {0, 1, 62, 63} and {(n - 1) >> 6 for n in QUERY_LENGTHS} == {2, 3, 4}
    notes = dict(cuts=[(k, c[0]) for k, c in enumerate(CUTS)], n_cut=len(CUTS), long_db=11, long_queries=LONG_QUERIES, no_t_db=10, all_t_query=10)
    return db, queries, notes


def pairs(db, queries, notes) -> list:
    """the full rectangle over the 11 database sequences in front of the long one, then the three pairs against it: 124 pairs (query,
    database sequence)"""
    out = [(q, d) for q in range(len(queries)) for d in range(notes["long_db"])] + [(q, notes["long_db"]) for q in notes["long_queries"]]
    assert len(out) == 11 * 11 + 3 == 124
    return out


def references(scoring, db, queries, which) -> dict:
    """(q, d) -> (want, flipped, last): the contract's result and what the other tie order and the other end-row rule would give,
    three walks over one fill"""
    out = {}
    codes_d, codes_q = [fit_ref.encode(scoring, s) for s in db], [fit_ref.encode(scoring, s) for s in queries]
    for q, d in which:
        tabs = fit_ref.fill(scoring, codes_d[d], codes_q[q])
        out[q, d] = tuple(fit_ref.fit_codes(scoring, codes_d[d], codes_q[q], flipped_ties=f, last_end_row=e, tabs=tabs)
                          for f, e in ((False, False), (True, False), (False, True)))
    return out


def covers_a_strip_edge(cigar) -> bool:
    """an I run holds columns 64 and 65, or 128 and 129, 192 and 193, 256 and 257"""
    c = 0
    for length, op in cigar:
        if op == "I" and any(c < edge < c + length for edge in STRIP_EDGES):  # columns c + 1 .. c + length
            return True
        if op != "D":
            c += length
    return False


def counts(ref: dict, db, queries) -> dict:
    """the conditions, counted over the pairs of `ref`"""
    n = dict(pairs=len(ref), cigar_flips=0, end_row_moves=0, begin_flips=0, edge_runs=0, inside=0, row0_runs=0)
    for (q, d), (want, flipped, last) in ref.items():
        assert flipped["score"] == last["score"] == want["score"] and flipped["db_end"] == want["db_end"]
        assert (last["db_end"] != want["db_end"]) == (want["plateau"] > 1)
        n["cigar_flips"] += flipped["cigar"] != want["cigar"]
        n["end_row_moves"] += last["db_end"] != want["db_end"]
        n["begin_flips"] += flipped["db_begin"] != want["db_begin"]
        n["edge_runs"] += want["db_begin"] > 0 and covers_a_strip_edge(want["cigar"])
        n["inside"] += 0 < want["db_begin"] and want["db_end"] < len(db[d])
        n["row0_runs"] += want["db_begin"] == 0 and want["cigar"][0][1] == "I" and want["cigar"][0][0] >= 65
    return n


def zero_gaps(gaps: dict) -> bool:
    return not any(gaps.get(k) for k in ("gap_pen", "gap_open", "gap_extend"))


def check_floors(n: dict, method: str, gaps: dict, begin_flips=None) -> None:
    """what a reference over this store must hold under one scoring; begin_flips: the count to ask for where a subset of the pairs
    cannot hold the share of the whole store (its caller says why)"""
    zero = zero_gaps(gaps)
    what = f"{method} {gaps}: {n}"
    assert 10 * n["cigar_flips"] >= 4 * n["pairs"], "the other tie order changes too few CIGARs: " + what
    assert n["end_row_moves"] >= 4 and (not zero or 10 * n["end_row_moves"] >= 4 * n["pairs"]), "too few plateaus in column n: " + what
    if zero and begin_flips is not None:
        assert n["begin_flips"] >= begin_flips > 0, "the other tie order moves too few db_begin: " + what
    elif zero and method == "nw":
        assert n["begin_flips"] >= 5, "the other tie order moves too few db_begin: " + what
    elif zero:
        assert 10 * n["begin_flips"] >= 2 * n["pairs"], "the other tie order moves too few db_begin: " + what
    else:
        assert n["edge_runs"] >= 8, "too few I runs over a strip edge with db_begin > 0: " + what
    assert 100 * n["inside"] >= 15 * n["pairs"], "too few pairs strictly inside: " + what
    assert n["row0_runs"] >= 2, "too few walks along row 0 over a strip edge: " + what


def check_all_t(ref: dict, scoring, notes: dict) -> None:
    """T x 193 against (ACG) x 40: nothing matches, the query does best against nothing -- border(193); the same run of 193 gaps
    starts from M[r][0] = 0 in every row, so all 121 rows of column n tie under every scoring and row 0 wins by the rule alone"""
    want = ref[notes["all_t_query"], notes["no_t_db"]][0]
    assert want["db_end"] == 0 and want["db_begin"] == 0 and want["score"] == fit_ref.row0(scoring, 193) and want["cigar"] == [(193, "I")]
    assert want["plateau"] == 121
