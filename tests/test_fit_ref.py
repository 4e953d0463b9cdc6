"""CPU: tests/fit_ref.py -- the plain-Python restatement of the fit contract the GPU tests compare against -- anchored at the
oracle: what the fit score means.  For short pairs the fit score must equal the largest global score of the query against any
substring of the database sequence, the empty substring (closed form: the query against gaps) included.  Every substring and the
query go through the oracle's alignment as one store; the query is its last sequence, so every pair (substring, query) is in the
canonical orientation of the contract."""
import numpy as np
import pytest

from tests import fit_ref

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
