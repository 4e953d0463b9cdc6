"""GPU (-m gpu): the fit sweep and the fitted tracebacks (sa_k_fit, the FIT forms of sa_k_trace_fill / sa_k_trace_walk; contract:
include/seqalign_hip.h, "queries fitted inside database sequences"), exactly, where the strips and the ties meet: queries of three to
five strips of 64 columns under seven scorings that tie everywhere.

tests/test_gpu_fit.py reaches a second to fourth strip only with random proteins under BLOSUM62 / 4 and / 10-1 -- hardly a tie, and
queries planted by substitution alone -- and runs its tie-heavy scorings inside strip 0.  What is device code of its own behind
strip 0 therefore decided nothing there: the boundary payload lines lane 63 writes and lane 0 of the next strip reads (M and X, the
third word `begin` in a buffer of its own), `begin` carried through the X state across columns 64 | 65, the end cell kept by a lane
of a later strip, the fitted walk's window over several strips and its run along row 0.  A wrong choice among equally good moves
still gives a valid alignment of the right score and a plausible span: only an exact comparison on inputs that tie can see it.

Inputs (tests/fit_strip_cases.py): four-letter DNA.  Database: random entries of 63, 64, 65, 130, 200, 257, 400, 700, the tandem
repeats (ACGT)^60 and ((AC)^40 GGT)^3, (ACG)^40 without a T, one entry of 3000.  Queries: five cut out of the 257, 400 and 700,
strictly inside, 129, 192, 193, 257 and 320 long -- 5 % substitutions, inserted runs of 2 to 10 over the strip edges, deletions of 5
to 7 --, the repeats (ACGT)^48 A, (AC)^128, ((AC)^40 GGT)^2 (AC)^12 A, random ones of 255 and 130, T^193: the end lane at 0, 1, 62
and 63 of the third to fifth strip.  The rectangle over the first 11 entries and three pairs against the 3000: 124 pairs.

Every expectation is tests/fit_ref.py (plain Python over full tables; no code shared with the library), computed once per scoring.
Sensitivity, from the reference alone and asserted before the device is asked (fit_strip_cases.check_floors): fit_ref walks the
same tables with the other order among equally good moves (flipped_ties) and takes the largest row among equal maxima of column n
(last_end_row); what those other rules would change is counted, so a device that follows them cannot pass.  Counts of this store, of
124 pairs (floors: CIGAR >= 40 %; end row >= 4, >= 40 % under zero gaps; db_begin >= 5 under NW 0, >= 20 % under Gotoh 0/0; an I run
over columns 64 | 65, 128 | 129, 192 | 193 or 256 | 257 with db_begin > 0 >= 8 under non-zero gaps; strictly inside >= 15 %; a leading
I run of >= 65 columns from db_begin = 0 -- the walk goes left along row 0 over a strip edge -- >= 2):

                        CIGAR differs   db_end moves    db_begin differs   I run over a    strictly   row 0 for
                        (other order)   (largest row)   (other order)      strip edge      inside     >= 65 columns
    nw +5/-4 gap 2 ....... 108 ............. 9 .............. 1 .............. 29 ........... 61 ......... 8
    nw +5/-4 gap 0 ........ 66 ............ 71 ............. 13 ............... 4 ........... 19 ........ 22
    nw +5/-4 gap 4 ........ 66 ............ 47 .............. 2 .............. 14 ........... 53 ........ 13
    ga +5/-4 3 / 1 ....... 115 ............ 13 .............. 1 .............. 36 ........... 58 ......... 4
    ga +5/-4 0 / 0 ....... 121 ............ 71 ............. 33 .............. 29 ........... 47 ......... 3
    ga +5/-4 3 / 7 ....... 120 ............ 16 .............. 1 .............. 29 ........... 63 ......... 8
    ga +5/-4 10 / 1 ...... 117 ............ 35 .............. 5 .............. 65 ........... 92 ......... 2

T^193 against (ACG)^40 matches nowhere: the run of 193 gaps starts from M[r][0] = 0 in every row, all 121 rows of column n tie
under every scoring, and the end row must be 0 by the rule alone (fit_strip_cases.check_all_t).

1. the rectangle, 11 x 11, six outputs, pid under two denominators
2. the list form over the 124 pairs, shuffled, the long rows first and last
3. alignments of the 124 pairs: records, CIGARs, spans equal to the kernel's, re-scored; three batches give the same bytes
4. a strands context over the cut-out queries: rows M .. 2 M through the three calls
5. the compositions of DESIGN 4.21: strand_fold over the halves of a fit rectangle, hits_above on one

Wall time of this file on the MI355X machine: 17 to 30 s over five runs, about 25 s typically.  The Python references take most of
it -- 2.5 to 5 s a scoring, about 28 s together on a slower host -- and the first test pays the start of the device; the device work of a
scoring is well under a second (the slowest test behind the first takes 2.3 s, reference included).
"""
import numpy as np
import pytest

from tests import fit_ref, fit_strip_cases
from tests.strands_cases import Folded, rc
from tests.test_gpu_fit import COLUMNS, LONGER, OUTPUTS, SHORTER, check_alignments, device_fit_pairs, device_fit_rect

pytestmark = pytest.mark.gpu

SCORINGS = [
    ("nw", dict(gap_pen=2)), ("nw", dict(gap_pen=0)), ("nw", dict(gap_pen=4)),
    ("ga", dict(gap_open=3, gap_extend=1)),
    ("ga", dict(gap_open=0, gap_extend=0, equal_affine_to_nw=False)),   # zero gaps
    ("ga", dict(gap_open=3, gap_extend=7)),                               # |open| < |extend|
    ("ga", dict(gap_open=10, gap_extend=1)),
]
STRAND_SCORINGS = [SCORINGS[0], SCORINGS[3]]
_ref, _strands = {}, {}


def scoring_id(v):
    return v if isinstance(v, str) else "-".join(str(x) for x in v.values() if x is not False)


def scoring_of(sa, method, gaps):
    """dnafull: +5 / -4 on A, C, G, T"""
    scoring = sa.Scoring.from_names(method, "dnafull", **gaps)
    codes = [int(scoring.lut[ch]) for ch in b"ACGT"]
    sub = np.asarray(scoring.sub).reshape(24, 24)[np.ix_(codes, codes)]
    assert len(set(codes)) == 4 and np.array_equal(sub, np.where(np.eye(4, dtype=bool), 5, -4))
    assert scoring.method == {"nw": fit_ref.NW, "ga": fit_ref.GA}[method]
    return scoring


def key_of(method, gaps):
    return method, tuple(sorted(gaps.items()))


class Nested:
    """res[q][d] over a dict keyed (q, d): what tests/test_gpu_fit.py: check_alignments indexes"""

    def __init__(self, ref):
        self.rows = {}
        for (q, d), (want, _, _) in ref.items():
            self.rows.setdefault(q, {})[d] = want

    def __getitem__(self, q):
        return self.rows[q]


def reference(sa, method, gaps):
    """the reference of one scoring over the 124 pairs, computed once, its conditions asserted: (ref, rectangle arrays 11 x 11, db,
    queries, notes, pairs, scoring)"""
    key = key_of(method, gaps)
    if key not in _ref:
        db, queries, notes = fit_strip_cases.strip_store()
        pairs = fit_strip_cases.pairs(db, queries, notes)
        scoring = scoring_of(sa, method, gaps)
        ref = fit_strip_cases.references(scoring, db, queries, pairs)
        n = fit_strip_cases.counts(ref, db, queries)
        print(f"{method} {gaps}: {n}")
        fit_strip_cases.check_floors(n, method, gaps)
        fit_strip_cases.check_all_t(ref, scoring, notes)
        nd, nq = notes["long_db"], len(queries)
        arr = {name: np.array([[ref[q, d][0][name] for d in range(nd)] for q in range(nq)], np.int64) for name in OUTPUTS[:5]}
        for a in arr.values():
            a.setflags(write=False)
        _ref[key] = (ref, arr, db, queries, notes, pairs, scoring)
    return _ref[key]


def pid_rect(arr, db, queries, denom):
    nq, nd = arr["score"].shape
    return np.array([[fit_ref.pid(int(arr["identities"][q, d]), int(arr["columns"][q, d]), len(db[d]), len(queries[q]), denom) for d in range(nd)]
                     for q in range(nq)], np.int64)


def same(what, got, want, ref_pairs, db, queries):
    """element t of got and want belongs to the pair ref_pairs[t]"""
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    if bad.size:
        q, d = ref_pairs[bad[0]]
        raise AssertionError(f"{what}: {bad.size} of {len(ref_pairs)} differ, first query {q} ({len(queries[q])} columns, end lane {(len(queries[q]) - 1) & 63} of strip "
                             f"{(len(queries[q]) - 1) >> 6}) database sequence {d} ({len(db[d])} rows): got {np.asarray(got).reshape(-1)[bad[0]]}, "
                             f"want {np.asarray(want).reshape(-1)[bad[0]]}")


# ---- 1. the rectangle --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,gaps", SCORINGS, ids=scoring_id)
def test_rectangle_past_strip_two_equals_the_python_restatement(method, gaps, sa):
    ref, arr, db, queries, notes, pairs, scoring = reference(sa, method, gaps)
    nd, nq = notes["long_db"], len(queries)
    block = [(q, d) for q in range(nq) for d in range(nd)]
    assert block == pairs[:nq * nd] and (nq, nd) == (11, 11)
    with sa.SearchContext(sa.SequenceStore.from_sequences(db[:nd]), sa.SequenceStore.from_sequences(queries), scoring, 0) as ctx:
        for denom in (COLUMNS, LONGER):
            got = device_fit_rect(ctx, 0, nq, nd, denom)
            for name in OUTPUTS[:5]:
                same(f"{method} {gaps} denom {denom} {name}", got[name], arr[name], block, db, queries)
            same(f"{method} {gaps} denom {denom} pid", got["pid"], pid_rect(arr, db, queries, denom), block, db, queries)


# ---- 2. the list form --------------------------------------------------------------------------------------------------------------------
def shuffled(pairs, notes, seed):
    """the pairs against the 3000-residue entry first (two) and last (one), the rest shuffled between them"""
    long = [p for p in pairs if p[1] == notes["long_db"]]
    rest = [p for p in pairs if p[1] != notes["long_db"]]
    assert len(long) == 3
    order = np.random.default_rng(seed).permutation(len(rest))
    return long[:2] + [rest[k] for k in order] + long[2:]


@pytest.mark.parametrize("method,gaps", SCORINGS, ids=scoring_id)
def test_list_form_past_strip_two(method, gaps, sa):
    ref, arr, db, queries, notes, pairs, scoring = reference(sa, method, gaps)
    items = shuffled(pairs, notes, 41)
    assert sorted(items) == sorted(pairs) and items != pairs and len(db[items[0][1]]) == len(db[items[-1][1]]) == fit_strip_cases.LONG
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0) as ctx:
        got = device_fit_pairs(ctx, [q for q, _ in items], [d for _, d in items], SHORTER)
    for name in OUTPUTS[:5]:
        same(f"{method} {gaps} {name}", got[name], [ref[p][0][name] for p in items], items, db, queries)
    want = [fit_ref.pid(ref[q, d][0]["identities"], ref[q, d][0]["columns"], len(db[d]), len(queries[q]), SHORTER) for q, d in items]
    same(f"{method} {gaps} pid", got["pid"], want, items, db, queries)


# ---- 3. alignments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,gaps", SCORINGS, ids=scoring_id)
def test_fitted_alignments_past_strip_two(method, gaps, sa, monkeypatch):
    from tests.test_gpu_wave_trips import pair_bytes
    ref, arr, db, queries, notes, pairs, scoring = reference(sa, method, gaps)
    items = shuffled(pairs, notes, 43)
    stores = sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries)
    with sa.SearchContext(*stores, scoring, 0) as ctx:
        device = device_fit_pairs(ctx, [q for q, _ in items], [d for _, d in items], want=("score", "db_begin", "db_end"))
        alns = ctx.fit_alignments(items)
        assert sa.last_alignments_breakdown()["batches"] == 1
    assert len(alns.records) == len(items)
    check_alignments(f"{method} {gaps}", alns, items, Nested(ref), db, queries, scoring, device)
    # once more, the decision scratch of a third of the pairs at a time: the same bytes
    total = sum(pair_bytes(len(db[d]), len(queries[q])) for q, d in items)
    monkeypatch.setenv("SA_HIP_TRACE_BATCH_BYTES", str(total // 3))  # (a context reads the switches when it is created)
    with sa.SearchContext(*stores, scoring, 0) as ctx:
        many = ctx.fit_alignments(items)
    assert sa.last_alignments_breakdown()["batches"] >= 3
    assert many.records.tobytes() == alns.records.tobytes() and many.cigar.tobytes() == alns.cigar.tobytes()


# ---- 4. a strands context ------------------------------------------------------------------------------------------------------------------
def strands_reference(sa, method, gaps):
    """the five cut-out queries and their reverse complements (written in Python) against the first 11 entries: (ref of the rows
    M + q keyed (q, d), arrays (M, 11), db, queries, reverse complements, scoring)"""
    key = key_of(method, gaps)
    if key not in _strands:
        _, _, db, queries, notes, _, scoring = reference(sa, method, gaps)
        db, cut = db[:notes["long_db"]], queries[:notes["n_cut"]]
        rev = [rc(s) for s in cut]
        assert all(len(a) == len(b) and a != b for a, b in zip(cut, rev))
        ref = fit_strip_cases.references(scoring, db, rev, [(q, d) for q in range(len(rev)) for d in range(len(db))])
        arr = {name: np.array([[ref[q, d][0][name] for d in range(len(db))] for q in range(len(rev))], np.int64) for name in OUTPUTS[:5]}
        for a in arr.values():
            a.setflags(write=False)
        _strands[key] = (ref, arr, db, cut, rev, scoring)
    return _strands[key]


@pytest.mark.parametrize("method,gaps", STRAND_SCORINGS, ids=scoring_id)
def test_strands_context_fits_the_reverse_complements_past_strip_two(method, gaps, sa):
    ref, arr, db, cut, rev, scoring = strands_reference(sa, method, gaps)
    fwd = reference(sa, method, gaps)[1]
    nd, m = len(db), len(cut)
    block = [(q, d) for q in range(m) for d in range(nd)]
    n = fit_strip_cases.counts(ref, db, rev)
    print(f"reverse complements, {method} {gaps}: {n}")
    assert 10 * n["cigar_flips"] >= 4 * n["pairs"] and n["end_row_moves"] >= 1, n   # (these rows tie as well; their queries are planted nowhere)
    items = [block[k] for k in np.random.default_rng(47).permutation(len(block))]
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(cut), scoring, 0, strands=True) as ctx:
        assert ctx.n_queries == 2 * m
        got = device_fit_rect(ctx, m, m, nd, LONGER)
        both = device_fit_rect(ctx, 0, 2 * m, nd, want=("score", "db_begin"))
        listed = device_fit_pairs(ctx, [m + q for q, _ in items], [d for _, d in items], COLUMNS)
        alns = ctx.fit_alignments([(m + q, d) for q, d in items])
    for name in OUTPUTS[:5]:
        same(f"strands {method} {gaps} rows M .. 2 M {name}", got[name], arr[name], block, db, rev)
        same(f"strands {method} {gaps} list {name}", listed[name], [ref[p][0][name] for p in items], items, db, rev)
    same(f"strands {method} {gaps} pid", got["pid"], pid_rect(arr, db, rev, LONGER), block, db, rev)
    same(f"strands {method} {gaps} list pid", listed["pid"], [fit_ref.pid(ref[q, d][0]["identities"], ref[q, d][0]["columns"], len(db[d]), len(rev[q]), COLUMNS) for q, d in items], items, db, rev)
    for name in ("score", "db_begin"):
        assert np.array_equal(both[name][:m], fwd[name][:m]) and np.array_equal(both[name][m:], arr[name]), f"strands {method} {gaps}: all 2 M rows, {name}"
    check_alignments(f"strands {method} {gaps}", alns, items, Nested(ref), db, rev, scoring, listed)


# ---- 5. compositions -----------------------------------------------------------------------------------------------------------------------
def test_strand_fold_over_the_halves_of_a_fit_rectangle(sa):
    import torch
    from tests.test_gpu_strands import Dev, bits_u64
    method, gaps = STRAND_SCORINGS[0]
    ref, arr, db, cut, rev, scoring = strands_reference(sa, method, gaps)
    nd, m = len(db), len(cut)
    exp = Folded(reference(sa, method, gaps)[1]["score"][:m].astype(np.int32), arr["score"].astype(np.int32))
    assert exp.strand.any() and not exp.strand.all(), "one strand only"
    assert all(not exp.strand[q, d] for q, d in reference(sa, method, gaps)[4]["cuts"]), "a cut-out query is found on its own strand"
    words = sa.strand_words(nd)
    dev = Dev(torch)
    prect, pbest, pbits = dev.new("rect", 2 * m * nd, torch.int32), dev.new("best", m * nd, torch.int32), dev.new("bits", m * words, torch.int64)
    torch.cuda.synchronize()
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(cut), scoring, 0, strands=True) as ctx:
        ctx.fit_rect(0, 2 * m, score=prect)
        ctx.strand_fold(prect, prect + 4 * m * nd, m, pbest, pbits)
        torch.cuda.synchronize()
    assert np.array_equal(dev.get("rect", (2 * m, nd)), np.concatenate([exp.fwd, exp.rev])), "the fit rectangle of both strands"
    assert np.array_equal(dev.get("best", (m, nd)), exp.best), "folded fit scores"
    assert np.array_equal(bits_u64(dev.get("bits", (m, words))), exp.bits()), "the strand bitmap"


def test_hits_above_on_a_fit_rectangle(sa):
    import torch
    from tests.test_gpu_search_above import assert_same_csr, expected_csr, run_above
    from tests.test_gpu_strands import Dev
    method, gaps = STRAND_SCORINGS[0]
    ref, arr, db, cut, rev, scoring = strands_reference(sa, method, gaps)
    nd, m = len(db), len(cut)
    rect = np.concatenate([reference(sa, method, gaps)[1]["score"][:m], arr["score"]]).astype(np.int32)
    t = int(np.sort(rect, axis=None)[rect.size // 2])   # the median (the upper one of an even count: an element of the rectangle)
    want = expected_csr(rect, rect, t)
    e = int(want[0][2 * m])
    assert 0 < e < rect.size and (rect == t).any(), "the median keeps a part, and the threshold itself is a value of the rectangle"
    dev = Dev(torch)
    prect = dev.new("rect", 2 * m * nd, torch.int32)
    torch.cuda.synchronize()
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(cut), scoring, 0, strands=True) as ctx:
        ctx.fit_rect(0, 2 * m, score=prect)
        torch.cuda.synchronize()
        got = run_above(sa, ctx, dev.bufs["rect"], dev.bufs["rect"], 2 * m, nd, t, e)
    assert_same_csr(got, want, f"fit scores >= {t}")
    assert np.array_equal(dev.get("rect", (2 * m, nd)), rect), "the fit rectangle was written"
