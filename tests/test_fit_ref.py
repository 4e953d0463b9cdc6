"""CPU: tests/fit_ref.py -- the plain-Python restatement of the fit contract the GPU tests compare against -- anchored at the
oracle: what the fit score means.  For short pairs the fit score must equal the largest global score of the query against any
substring of the database sequence, the empty substring (closed form: the query against gaps) included.  Every substring and the
query go through the oracle's alignment as one store; the query is its last sequence, so every pair (substring, query) is in the
canonical orientation of the contract.

And the conditions of tests/test_gpu_fit_strips.py where no GPU runs: the store of tests/fit_strip_cases.py must keep its ties,
plateaus, strip-edge runs and row-0 walks under the reference, or that file compares the device on inputs that decide nothing."""
import types

import numpy as np
import pytest

from tests import fit_ref, fit_strip_cases

SCORINGS = [("nw", dict(gap_pen=4)), ("ga", dict(gap_open=10, gap_extend=1)), ("ga", dict(gap_open=3, gap_extend=7)), ("nw", dict(gap_pen=1))]
LETTERS = b"ACDEW"  # few letters: ties; C / E scores -4


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for k in range(10):
        m, n = int(rng.integers(1, 17)), int(rng.integers(1, 13))
        if k == 0:
            m, n = 16, 12
        if k == 1:
            m, n = 1, 12
        db = bytes(LETTERS[i] for i in rng.integers(0, len(LETTERS), m))
        qy = bytes(LETTERS[i] for i in rng.integers(0, len(LETTERS), n))
        if k % 2 and m > n + 1:
            s = int(rng.integers(1, m - n))
            qy = db[s:s + n]
        out.append((db, qy))
    out.append((b"E", b"CCCCC"))  # the query against nothing
    return out


@pytest.mark.parametrize("method,gaps", SCORINGS, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_fit_score_is_the_best_global_score_over_substrings(method, gaps, sa, oracle):
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    end0 = inside = 0
    for db, qy in cases():
        m = len(db)
        subs = [db[s:e] for s in range(m) for e in range(s + 1, m + 1)]
        store = sa.SequenceStore.from_sequences(subs + [qy])
        tri = oracle.align(store, scoring, triangular=True)
        j = len(subs)
        column = tri[j * (j - 1) // 2: j * (j - 1) // 2 + j]  # pairs (i, j), i < j: substring i the rows, the query the columns
        want = max(fit_ref.row0(scoring, len(qy)), int(column.max()))
        got = fit_ref.fit_pair(scoring, db, qy)
        assert got["score"] == want, f"{method} {gaps}: {db!r} / {qy!r}: fit {got['score']}, the best substring {want}"
        # the span the walk reports is a substring that reaches the score, and the CIGAR is priced at it
        if got["db_end"] > got["db_begin"]:
            assert int(column[subs.index(db[got["db_begin"]:got["db_end"]])]) == want
        else:
            assert want == fit_ref.row0(scoring, len(qy))
        assert fit_ref.rescore(scoring, db, qy, got) == want
        # the plain global recurrence of this file is the oracle's
        cd, cq = fit_ref.encode(scoring, db), fit_ref.encode(scoring, qy)
        assert fit_ref.global_score(scoring, cd, cq) == int(column[subs.index(db)])
        end0 += got["db_end"] == 0
        inside += got["db_begin"] > 0 and got["db_end"] < m
    assert end0 >= 1 and inside >= 2


# ---- the strip store keeps its conditions ------------------------------------------------------------------------------------------------
def plus5_minus4(method: str, gaps: dict):
    """a stand-in for a Scoring, fit_ref needs no library: A, C, G, T -> 0 .. 3, +5 / -4, the gaps negative as the library holds them"""
    lut = np.full(128, -1, np.int32)
    for code, ch in enumerate(b"ACGT"):
        lut[ch] = code
    sub = np.full((24, 24), -4, np.int32)
    np.fill_diagonal(sub, 5)
    return types.SimpleNamespace(lut=lut, sub=sub.reshape(-1), method={"nw": fit_ref.NW, "ga": fit_ref.GA}[method], gap_pen=-gaps.get("gap_pen", 0),
                                 gap_opn=-gaps.get("gap_open", 0), gap_ext=-gaps.get("gap_extend", 0))


@pytest.mark.parametrize("method,gaps,begin_flips", [("nw", dict(gap_pen=2), None), ("ga", dict(gap_open=0, gap_extend=0), 16)], ids=["nw-2", "ga-0-0"])
def test_strip_store_keeps_its_conditions(method, gaps, begin_flips):
    """The floors of tests/test_gpu_fit_strips.py on the 99 pairs with m <= 257 (a few seconds of Python), two of its seven scorings.
    Counts of these pairs (of 99): NW 2: CIGAR flips 83, end-row moves 6, strip-edge runs 24, inside 38, row-0 runs 8; Gotoh 0/0: 96, 49,
    db_begin flips 16, inside 29, row-0 runs 3.  One floor is lower here than over the whole store: under Gotoh 0/0 the other tie order
    moves db_begin in 33 of the 124 pairs (the floor is 20 %), but 17 of those are against the entries of 400, 700 and 3000 residues,
    where a query has room to start elsewhere; the 99 pairs left hold 16, and 16 is asked for."""
    db, queries, notes = fit_strip_cases.strip_store()
    scoring = plus5_minus4(method, gaps)
    which = [(q, d) for q, d in fit_strip_cases.pairs(db, queries, notes) if len(db[d]) <= 257]
    assert len(which) == 99
    ref = fit_strip_cases.references(scoring, db, queries, which)
    n = fit_strip_cases.counts(ref, db, queries)
    print(f"{method} {gaps}: {n}")
    fit_strip_cases.check_floors(n, method, gaps, begin_flips)
    fit_strip_cases.check_all_t(ref, scoring, notes)
    for (q, d), (want, flipped, last) in ref.items():  # the other rules give alignments of the same score: only an exact comparison tells them apart
        for res in (want, flipped, last):
            assert fit_ref.rescore(scoring, db[d], queries[q], res) == want["score"]
