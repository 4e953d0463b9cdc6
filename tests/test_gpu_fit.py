"""GPU (-m gpu): queries fitted inside database sequences -- the whole query against the best substring of the database sequence
(sa_ctx_fit_rect / sa_ctx_fit_pairs / sa_ctx_fit_alignments / sa_hip_search_fit, csrc/sa_fit.hip, the FIT forms of
csrc/sa_traceback.hip).  Contract: include/seqalign_hip.h, "queries fitted inside database sequences".

The expectation never comes from the code under test: tests/fit_ref.py (plain Python, pinned to the oracle by
tests/test_fit_ref.py) for every output, NumPy's lexsort for the hits, the oracle's NW and SW rectangles as bounds on larger
shapes.  Everything is compared exactly.

1. the rectangle against fit_ref, all six outputs, eight scorings
2. the list form: shuffled with repeats, indices out of range, later trips of the wavefronts
3. alignments: records and CIGARs against the fit_ref walk, re-scored, in batches
4. the one call: hits by score and by identity with ties across the cut, in batches
5. NW <= fit <= SW on larger shapes
6. nothing else moved; a strands context"""
import numpy as np
import pytest

from tests import fit_ref, tables
from tests.search_cases import expected_hits, oracle_rect
from tests.synth import make_dna_set, make_protein_set
from tests.test_gpu_wave_trips import resident_waves

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B
INT32_MIN = -(1 << 31)
COLUMNS, SHORTER, LONGER, MEAN = 0, 1, 2, 3
OUTPUTS = ("score", "db_begin", "db_end", "identities", "columns", "pid")


# ---- the stores ------------------------------------------------------------------------------------------------------------------------
def planted(source: bytes, start: int, length: int, seed: int, letters: bytes = b"ARNDCQEGHILKMFPSTWYV") -> bytes:
    """source[start, start + length) with about one residue in ten substituted"""
    rng = np.random.default_rng(seed)
    part = bytearray(source[start:start + length])
    for k in range(length):
        if rng.integers(10) == 0:
            part[k] = letters[rng.integers(len(letters))]
    return bytes(part)


def full_store():
    """(db, queries, planted pairs): database lengths {1, 2, 63, 64, 65, 130, 200} twice, N = 14; query lengths {1, 5, 63, 64, 65, 128,
    129, 200} -- the end lane at 0, 4, 62, 63, then the first and the last lane of a second strip, and into a third and a fourth
    strip.  Four queries are substrings of a database sequence, strictly inside it.  The database sequences of one and two residues
    are E and the query of five residues is CCCCC (BLOSUM62: -4 a column): against them the query does best against nothing."""
    lens = [1, 2, 63, 64, 65, 130, 200]
    db = [make_protein_set(1, ln, ln, 900 + 7 * k + ln)[0] for k in range(2) for ln in lens]
    db[0], db[1], db[7], db[8] = b"E", b"EE", b"E", b"EW"
    queries = [make_protein_set(1, ln, ln, 1300 + ln)[0] for ln in (1, 5, 63, 64, 65, 128, 129, 200)]
    queries[1] = b"CCCCC"
    plants = [(2, 6, 31, 63), (3, 13, 100, 64), (5, 6, 40, 128), (6, 13, 1, 129)]  # (query, database sequence, start, length)
    for q, d, start, length in plants:
        assert 0 < start and start + length < len(db[d])
        queries[q] = planted(db[d], start, length, 50 + q)
    assert [len(s) for s in queries] == [1, 5, 63, 64, 65, 128, 129, 200] and [len(s) for s in db] == lens * 2
    return db, queries, [(q, d) for q, d, _, _ in plants]


def reduced_store():
    """lengths <= 70, N = 8, M = 4; two planted queries; E / EE against CCCCC as above"""
    db = [b"E", b"EE"] + [make_protein_set(1, ln, ln, 400 + ln)[0] for ln in (7, 33, 63, 64, 65, 70)]
    queries = [b"W", b"CCCCC", planted(db[7], 3, 64, 9), planted(db[6], 1, 20, 10)]
    return db, queries, [(2, 7), (3, 6)]


def all_mismatch_table():
    """every mismatch -100, every match 2"""
    sub = np.full((24, 24), -100, np.int32)
    np.fill_diagonal(sub, 2)
    return sub


def scoring_of(sa, spec):
    method, table, gaps = spec
    if table == "blosum62":
        return sa.Scoring.from_names(method, "blosum62", **gaps)
    sub = tables.asym() if table == "asym" else all_mismatch_table()
    return tables.scoring_with(sa, method, gaps, sub, lut=sa.Scoring.from_names(method, "blosum62", **gaps).lut)


FULL_SCORINGS = [("nw", "blosum62", dict(gap_pen=4)), ("ga", "blosum62", dict(gap_open=10, gap_extend=1))]
REDUCED_SCORINGS = [("nw", "blosum62", dict(gap_pen=0)), ("ga", "blosum62", dict(gap_open=0, gap_extend=0, equal_affine_to_nw=False)),
                    ("ga", "blosum62", dict(gap_open=3, gap_extend=7)), ("nw", "asym", dict(gap_pen=4)), ("ga", "asym", dict(gap_open=10, gap_extend=1)),
                    ("nw", "mismatch-100", dict(gap_pen=1))]
_ref = {}


def reference(sa, spec, which):
    """the reference of one scoring over a store, computed once: dict of (M, N) int64 arrays, the per-pair results, the store"""
    key = (spec[0], spec[1], tuple(sorted(spec[2].items())), which)
    if key not in _ref:
        db, queries, plants = full_store() if which == "full" else reduced_store()
        scoring = scoring_of(sa, spec)
        res = [[fit_ref.fit_pair(scoring, d, q) for d in db] for q in queries]
        arr = {name: np.array([[r[name] for r in row] for row in res], np.int64) for name in OUTPUTS[:5]}
        for a in arr.values():
            a.setflags(write=False)
        _ref[key] = (arr, res, db, queries, plants, scoring)
    return _ref[key]


def pid_of(arr, db, queries, denom):
    return np.array([[fit_ref.pid(int(arr["identities"][q, d]), int(arr["columns"][q, d]), len(db[d]), len(queries[q]), denom) for d in range(len(db))]
                     for q in range(len(queries))], np.int64)


def device_fit_rect(ctx, q0, nq, n, denom=COLUMNS, want=OUTPUTS, stream=0):
    """the outputs asked for, each between a poisoned row before and 64 poisoned elements behind"""
    import torch
    count = nq * n
    bufs = {name: torch.full((n + count + 64,), POISON, dtype=torch.int32, device="cuda") for name in want}
    torch.cuda.synchronize()
    ctx.fit_rect(q0, nq, denom=denom, stream=stream, **{name: b.data_ptr() + 4 * n for name, b in bufs.items()})
    torch.cuda.synchronize()
    got = {}
    for name, b in bufs.items():
        host = b.cpu().numpy()
        assert (host[:n] == POISON).all() and (host[n + count:] == POISON).all(), f"sa_ctx_fit_rect wrote outside the rows in {name}"
        got[name] = host[n:n + count].reshape(nq, n).copy()
    return got


def device_fit_pairs(ctx, query, db, denom=COLUMNS, want=OUTPUTS, stream=0):
    import torch
    count = len(query)
    d_q, d_d = torch.from_numpy(np.asarray(query, np.int32)).cuda(), torch.from_numpy(np.asarray(db, np.int32)).cuda()
    bufs = {name: torch.full((16 + count + 64,), POISON, dtype=torch.int32, device="cuda") for name in want}
    torch.cuda.synchronize()
    ctx.fit_pairs(d_q.data_ptr(), d_d.data_ptr(), count, denom=denom, stream=stream, **{name: b.data_ptr() + 64 for name, b in bufs.items()})
    torch.cuda.synchronize()
    got = {}
    for name, b in bufs.items():
        host = b.cpu().numpy()
        assert (host[:16] == POISON).all() and (host[16 + count:] == POISON).all(), f"sa_ctx_fit_pairs wrote outside the items in {name}"
        got[name] = host[16:16 + count].copy()
    return got


def compare(what, got, want, db, queries):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {want.size} differ, first query {bad[0][0]} d {bad[0][1]} ({len(db[bad[0][1]])} x "
                           f"{len(queries[bad[0][0]])} residues): got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


# ---- 1. the rectangle against fit_ref ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,which", [(s, "full") for s in FULL_SCORINGS] + [(s, "reduced") for s in REDUCED_SCORINGS],
                         ids=lambda v: v if isinstance(v, str) else "-".join([v[0], v[1]] + [str(x) for x in v[2].values()]))
def test_rectangle_equals_the_python_restatement(spec, which, sa):
    arr, res, db, queries, plants, scoring = reference(sa, spec, which)
    n, m = len(db), len(queries)
    assert (n, m) == ((14, 8) if which == "full" else (8, 4))
    # what the case must hold, asserted on the expectation
    if spec[1] != "asym":  # (E against C: -4 under BLOSUM62, -100 under the all-mismatch table; the asymmetric table promises no such pair)
        assert (arr["db_end"] == 0).any(), "no pair ends at row 0"
    assert any(len(db[d]) < len(queries[q]) for q in range(m) for d in range(n))
    inside = sum(1 for q, d in plants if arr["db_begin"][q, d] > 0 and arr["db_end"][q, d] < len(db[d]))
    assert 4 * inside >= len(plants) and inside >= 1, "the planted queries do not sit strictly inside"
    assert (arr["db_begin"] <= arr["db_end"]).all() and (arr["db_begin"] >= 0).all()
    assert all(arr["db_end"][q, d] <= len(db[d]) for q in range(m) for d in range(n))
    if spec[1] == "mismatch-100":
        # CCCCC against E and EE: no match anywhere, the query against gaps ties with every row, the end row is 0
        for d in (0, 1):
            M = fit_ref.fill(scoring, fit_ref.encode(scoring, db[d]), fit_ref.encode(scoring, queries[1]))[0]
            assert all(row[5] == -5 for row in M) and arr["db_end"][1, d] == 0 and arr["score"][1, d] == -5
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0) as ctx:
        for denom in (COLUMNS, SHORTER, LONGER, MEAN):  # (on stream 0; a side stream: tests/test_gpu_fit_stream_order.py)
            got = device_fit_rect(ctx, 0, m, n, denom)
            for name in OUTPUTS[:5]:
                compare(f"{spec} denom {denom} {name}", got[name], arr[name], db, queries)
            compare(f"{spec} denom {denom} pid", got["pid"], pid_of(arr, db, queries, denom), db, queries)
        # subsets of the outputs, q0 > 0
        for q0, nq, names in ((1, 1, ("db_begin",)), (m - 2, 2, ("score", "db_end")), (1, m - 1, ("pid", "columns"))):
            got = device_fit_rect(ctx, q0, nq, n, LONGER, names)
            for name in names:
                want = pid_of(arr, db, queries, LONGER) if name == "pid" else arr[name]
                assert np.array_equal(got[name], want[q0:q0 + nq]), f"queries [{q0},+{nq}) {name}"


def test_refusals_of_the_fit_calls(sa):
    """every refusal with its message, nothing launched (the poison stays), each followed by a valid call"""
    import torch
    arr, res, db, queries, plants, scoring = reference(sa, REDUCED_SCORINGS[0], "reduced")
    n, m = len(db), len(queries)
    stores = sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries)
    d_out = torch.full((m * n + 8,), POISON, dtype=torch.int32, device="cuda")
    d_idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    o, x = d_out.data_ptr(), d_idx.data_ptr()
    with sa.SearchContext(*stores, scoring, 0) as ctx:
        refusals = [
            ("sa_ctx_fit_rect: every output is null", lambda: ctx.fit_rect(0, m)),
            ("sa_ctx_fit_rect: denom 4 is none of", lambda: ctx.fit_rect(0, m, pid=o, denom=4)),
            (r"sa_ctx_fit_rect: queries \[3,\+2\) of 4", lambda: ctx.fit_rect(3, 2, score=o)),
            (r"sa_ctx_fit_rect: queries \[0,\+0\) of 4", lambda: ctx.fit_rect(0, 0, score=o)),
            (r"sa_ctx_fit_rect: queries \[-1,\+1\) of 4", lambda: ctx.fit_rect(-1, 1, score=o)),
            ("sa_ctx_fit_rect: the outputs want 4-byte alignment", lambda: ctx.fit_rect(0, 1, db_begin=o + 2)),
            ("sa_ctx_fit_pairs: every output is null", lambda: ctx.fit_pairs(x, x, 4)),
            ("sa_ctx_fit_pairs: npairs = -1", lambda: ctx.fit_pairs(x, x, -1, score=o)),
            ("sa_ctx_fit_pairs: null index array", lambda: ctx.fit_pairs(0, x, 4, score=o)),
            ("sa_ctx_fit_pairs: null index array", lambda: ctx.fit_pairs(x, 0, 4, score=o)),
            ("sa_ctx_fit_pairs: d_query and d_db want 4-byte alignment", lambda: ctx.fit_pairs(x + 2, x, 1, score=o)),
            ("sa_ctx_fit_pairs: denom -1 is none of", lambda: ctx.fit_pairs(x, x, 4, pid=o, denom=-1)),
        ]
        for message, call in refusals:
            with pytest.raises(sa.AlignError, match=message):
                call()
            torch.cuda.synchronize()
            assert (d_out.cpu().numpy() == POISON).all(), f"{message}: something was launched"
            ctx.fit_rect(0, m, score=o)
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy()[:m * n].reshape(m, n), arr["score"])
            d_out.fill_(POISON)
            torch.cuda.synchronize()
        ctx.fit_pairs(0, 0, 0, score=o)  # no pairs: valid, nothing launched
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == POISON).all()
    sw = sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1)
    with sa.SearchContext(*stores, sw, 0) as ctx:
        for call in (lambda: ctx.fit_rect(0, m, score=o), lambda: ctx.fit_pairs(x, x, 4, score=o)):
            with pytest.raises(sa.AlignError, match="the context's method is SW"):
                call()
    with sa.Context(sa.SequenceStore.from_sequences([b"A"] * 8), scoring, 0) as plain:
        for call in (lambda: sa.SearchContext.fit_rect(plain, 0, 1, score=o), lambda: sa.SearchContext.fit_pairs(plain, x, x, 1, score=o)):
            with pytest.raises(sa.AlignError, match="not a search context"):
                call()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == POISON).all()


# ---- 2. the list form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", FULL_SCORINGS, ids=lambda v: v[0])
def test_list_form_gives_the_elements_of_the_rectangle(spec, sa):
    arr, res, db, queries, plants, scoring = reference(sa, spec, "full")
    n, m = len(db), len(queries)
    rng = np.random.default_rng(17)
    q = rng.integers(0, m, 300).astype(np.int32)
    d = rng.integers(0, n, 300).astype(np.int32)
    assert len({(a, b) for a, b in zip(q.tolist(), d.tolist())}) < 300  # repeats
    bad = {5: (m, 0), 77: (0, n), 150: (-1, 3), 299: (2, -1)}  # out of range: INT32_MIN, nothing read
    for at, (bq, bd) in bad.items():
        q[at], d[at] = bq, bd
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0) as ctx:
        got = device_fit_pairs(ctx, q, d, SHORTER)
        only = device_fit_pairs(ctx, q, d, want=("db_begin", "db_end"))
    pid = pid_of(arr, db, queries, SHORTER)
    for t in range(300):
        for name in OUTPUTS:
            want = INT32_MIN if t in bad else (pid if name == "pid" else arr[name])[q[t], d[t]]
            assert got[name][t] == want, f"{spec} item {t} (query {q[t]}, d {d[t]}) {name}: got {got[name][t]}, want {want}"
    assert np.array_equal(only["db_begin"], got["db_begin"]) and np.array_equal(only["db_end"], got["db_end"])


@pytest.mark.parametrize("method", ["nw", "ga"])
def test_list_form_on_later_trips(method, sa):
    """3 queries x enough database sequences of 3 .. 12 residues that the items pass twice the resident waves"""
    w = resident_waves()
    n = 2 * w // 3 + 40
    assert 3 * n > 2 * w
    distinct = [make_protein_set(1, 3 + k % 10, 3 + k % 10, 7000 + k)[0] for k in range(30)]
    order = np.random.default_rng(23).integers(0, 30, n)
    db = [distinct[k] for k in order]
    queries = [distinct[4][1:], make_protein_set(1, 9, 9, 61)[0], distinct[17][:-1] + b"W"]
    scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
    ref = [[fit_ref.fit_pair(scoring, s, qs) for s in distinct] for qs in queries]
    assert any(r["db_begin"] > 0 for row in ref for r in row) and any(r["db_end"] < len(distinct[k]) for row in ref for k, r in enumerate(row))
    q = np.repeat(np.arange(3, dtype=np.int32), n)
    d = np.tile(np.arange(n, dtype=np.int32), 3)
    perm = np.random.default_rng(29).permutation(3 * n)
    q, d = q[perm], d[perm]
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0) as ctx:
        got = device_fit_pairs(ctx, q, d, MEAN)
        rect = device_fit_rect(ctx, 0, 3, n, MEAN)
    for name in OUTPUTS:
        if name == "pid":
            want = np.array([fit_ref.pid(ref[a][order[b]]["identities"], ref[a][order[b]]["columns"], len(db[b]), len(queries[a]), MEAN)
                             for a, b in zip(q, d)], np.int64)
        else:
            want = np.array([ref[a][order[b]][name] for a, b in zip(q, d)], np.int64)
        bad = np.flatnonzero(got[name] != want)
        assert bad.size == 0, (f"{method} {name}: {bad.size} of {3 * n} items differ, first item {bad[0]} ({w} resident waves): got {got[name][bad[0]]}, "
                               f"want {want[bad[0]]}")
        assert np.array_equal(rect[name][q, d], want), f"{method} {name}: the rectangle on later trips"


# ---- 3. alignments -------------------------------------------------------------------------------------------------------------------------
def check_alignments(what, alns, pairs, res, db, queries, scoring, device):
    for t, (q, d) in enumerate(pairs):
        rec, want = alns.records[t], res[q][d]
        got = (int(rec["score"]), int(rec["a_begin"]), int(rec["a_end"]), int(rec["b_begin"]), int(rec["b_end"]), int(rec["columns"]), int(rec["identities"]))
        exp = (want["score"], 0, len(queries[q]), want["db_begin"], want["db_end"], want["columns"], want["identities"])
        assert got == exp, f"{what} pair {t} (query {q}, d {d}): record {got}, want {exp}"
        runs = alns.runs(t)
        assert runs == want["cigar"], f"{what} pair {t} (query {q}, d {d}): CIGAR {runs}, want {want['cigar']}"
        # the span is the kernel's for the same pair, and the CIGAR as written scores `score`
        assert (got[3], got[4], got[0]) == (device["db_begin"][t], device["db_end"][t], device["score"][t])
        assert fit_ref.rescore(scoring, db[d], queries[q], dict(db_begin=got[3], db_end=got[4], cigar=runs)) == got[0], f"{what} pair {t}: re-scored"


@pytest.mark.parametrize("spec", FULL_SCORINGS + [REDUCED_SCORINGS[2], REDUCED_SCORINGS[5]], ids=lambda v: "-".join([v[0], v[1]] + [str(x) for x in v[2].values()]))
def test_alignments_equal_the_walk(spec, sa, monkeypatch):
    from tests.test_gpu_wave_trips import pair_bytes
    which = "full" if spec in FULL_SCORINGS else "reduced"
    arr, res, db, queries, plants, scoring = reference(sa, spec, which)
    n, m = len(db), len(queries)
    order = np.random.default_rng(31).permutation(n * m)
    pairs = [(int(t) // n, int(t) % n) for t in order] + [plants[0], plants[0], (1, 0)]  # every pair, shuffled, and repeats
    assert any(res[q][d]["db_end"] == 0 for q, d in pairs) and any(len(r["cigar"]) > 3 for row in res for r in row)
    stores = sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries)
    q_of, d_of = [p[0] for p in pairs], [p[1] for p in pairs]
    with sa.SearchContext(*stores, scoring, 0) as ctx:
        device = device_fit_pairs(ctx, q_of, d_of, want=("score", "db_begin", "db_end"))
        alns = ctx.fit_alignments(pairs)
        assert sa.last_alignments_breakdown()["batches"] == 1
        assert len(ctx.fit_alignments([]).records) == 0
        for message, bad in (("index out of range", [(m, 0)]), ("index out of range", [(0, n)]), ("index out of range", [(0, 0), (-1, 0)])):
            with pytest.raises(sa.AlignError, match="sa_ctx_fit_alignments: pair .*" + message):
                ctx.fit_alignments(bad)
    check_alignments(str(spec), alns, pairs, res, db, queries, scoring, device)
    if which == "full":  # once more in batches: the decision scratch of a third of the pairs at a time
        total = sum(pair_bytes(len(db[d]), len(queries[q])) for q, d in pairs)
        monkeypatch.setenv("SA_HIP_TRACE_BATCH_BYTES", str(total // 3))  # (a context reads the switches when it is created)
        with sa.SearchContext(*stores, scoring, 0) as ctx:
            many = ctx.fit_alignments(pairs)
        assert sa.last_alignments_breakdown()["batches"] >= 3
        assert many.records.tobytes() == alns.records.tobytes() and many.cigar.tobytes() == alns.cigar.tobytes()


def test_fit_alignments_are_refused_where_fit_is(sa):
    db, queries, _ = reduced_store()
    stores = sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries)
    with sa.SearchContext(*stores, sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1), 0) as ctx:
        with pytest.raises(sa.AlignError, match="sa_ctx_fit_alignments: the context's method is SW"):
            ctx.fit_alignments([(0, 0)])
    with sa.Context(stores[0], sa.Scoring.from_names("nw", "blosum62", gap_pen=4), 0) as plain:
        with pytest.raises(sa.AlignError, match="sa_ctx_fit_alignments: not a search context"):
            sa.SearchContext.fit_alignments(plain, [(0, 0)])


# ---- 4. the one call -----------------------------------------------------------------------------------------------------------------------
_search = {}


def search_case(sa):
    """20 distinct database sequences each present twice under a fixed shuffle (ties cross every odd cut), 9 queries, four of them
    planted; NW / BLOSUM62 / 4; the reference's rectangles, computed once"""
    if not _search:
        distinct = make_protein_set(20, 20, 60, 71)
        db = [distinct[k] for k in np.random.default_rng(5).permutation(np.repeat(np.arange(20), 2))]
        queries = make_protein_set(9, 10, 30, 72)
        for q in (1, 3, 5, 7):
            src = distinct[q]
            queries[q] = planted(src, 2, min(len(queries[q]), len(src) - 4), 80 + q)
        scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
        res = [[fit_ref.fit_pair(scoring, d, q) for d in db] for q in queries]
        arr = {name: np.array([[r[name] for r in row] for row in res], np.int64) for name in OUTPUTS[:5]}
        _search["case"] = (db, queries, scoring, arr)
    return _search["case"]


def check_search(sa, what, got, arr, vrect, k):
    index, value, score, begin, end, got_rect, got_vrect = got
    rect = arr["score"]
    assert np.array_equal(got_rect, rect), f"{what}: rect"
    assert np.array_equal(got_vrect, vrect), f"{what}: vrect"
    wi, wv = expected_hits(vrect.astype(np.int32), k)
    at = wi.astype(np.int64)
    for name, g, w in (("index", index, wi), ("value", value, wv), ("score", score, np.take_along_axis(rect, at, 1)),
                       ("db_begin", begin, np.take_along_axis(arr["db_begin"], at, 1)), ("db_end", end, np.take_along_axis(arr["db_end"], at, 1))):
        assert g.dtype == np.int32 and g.shape == wi.shape, f"{what} k={k} {name}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} k={k} {name}: {len(bad)} entries differ, first at query {bad[0][0]} place {bad[0][1]}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
    return wi


@pytest.mark.parametrize("by", ["score", "identity-shorter"])
def test_one_call_hits(by, sa, monkeypatch):
    db, queries, scoring, arr = search_case(sa)
    n, m = len(db), len(queries)
    vrect = arr["score"] if by == "score" else pid_of(arr, db, queries, SHORTER)
    best = -np.sort(-vrect, axis=1)
    for k in (1, 5, 7):  # every value occurs an even number of times: for odd k every row ties across the cut
        assert (best[:, k - 1] == best[:, k]).all()
    stores = sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries)
    pid = None if by == "score" else SHORTER
    first = {}
    for k in (1, 5, 7, 8, n):
        first[k] = sa.hip_search_fit(*stores, scoring, k=k, rect=True, pid=pid)
        check_search(sa, by, first[k], arr, vrect, k)
        assert sa.last_search_breakdown()["batches"] == 1 and sa.last_search_fit_seconds() > 0
    if by != "score":
        assert (expected_hits(vrect.astype(np.int32), 7)[0] != expected_hits(arr["score"].astype(np.int32), 7)[0]).any(), "the two rankings agree"
    # the hits alone, the rectangles alone
    alone = sa.hip_search_fit(*stores, scoring, k=5, pid=pid)
    assert len(alone) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(alone, first[5][:5]))
    rects = sa.hip_search_fit(*stores, scoring, rect=True, pid=pid)
    assert len(rects) == 2 and rects[0].tobytes() == first[5][5].tobytes() and rects[1].tobytes() == first[5][6].tobytes()
    # three batches of three queries: the same bytes
    k = 7
    monkeypatch.setenv("SA_HIP_SEARCH_BATCH_BYTES", str(3 * (8 * n + 32 * k)))  # (include/seqalign_hip.h: sa_hip_search_fit)
    many = sa.hip_search_fit(*stores, scoring, k=k, rect=True, pid=pid)
    assert sa.last_search_breakdown()["batches"] == 3
    for a, b in zip(first[k], many):
        assert a.tobytes() == b.tobytes()


# ---- 5. anchors at the oracle on larger shapes ---------------------------------------------------------------------------------------------
def test_global_at_most_fit_at_most_local(sa, oracle):
    db = make_protein_set(40, 300, 700, 41)
    queries = make_protein_set(6, 64, 150, 42)
    queries[1] = planted(db[3], 100, 120, 1)
    queries[4] = planted(db[20], 250, 64, 2)
    stores = sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries)
    n, m = len(db), len(queries)
    nw = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    ga = sa.Scoring.from_names("ga", "blosum62", gap_open=10, gap_extend=1)
    sw = sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1)
    with sa.SearchContext(*stores, nw, 0) as ctx:
        fit_nw = device_fit_rect(ctx, 0, m, n, want=("score",))
    lower = oracle_rect(sa, oracle, db, queries, nw)
    assert (lower <= fit_nw["score"]).all() and (lower < fit_nw["score"]).any()
    with sa.SearchContext(*stores, ga, 0) as ctx:
        fit_ga = device_fit_rect(ctx, 0, m, n, want=("score",))["score"]
    upper = oracle_rect(sa, oracle, db, queries, sw)
    assert (fit_ga <= upper).all() and (fit_ga < upper).any()
    assert (oracle_rect(sa, oracle, db, queries, ga) <= fit_ga).all()


# ---- 6. nothing else moved; a strands context ------------------------------------------------------------------------------------------------
def test_the_other_calls_give_the_same_bytes_around_a_fit_call(sa):
    import torch
    arr, res, db, queries, plants, scoring = reference(sa, FULL_SCORINGS[1], "full")
    n, m = len(db), len(queries)
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0) as ctx:
        def others():
            rect = torch.full((m * n,), POISON, dtype=torch.int32, device="cuda")
            scratch = torch.empty(ctx.search_scratch_bytes(0, m) + 8, dtype=torch.uint8, device="cuda")
            ident = {name: torch.full((m * n,), POISON, dtype=torch.int32, device="cuda") for name in ("score", "identities", "columns", "pid")}
            ctx.search_range(0, m, rect.data_ptr(), scratch.data_ptr())
            torch.cuda.synchronize()
            ctx.identity_rect(0, m, denom=MEAN, **{name: b.data_ptr() for name, b in ident.items()})
            torch.cuda.synchronize()
            return [rect.cpu().numpy().tobytes()] + [b.cpu().numpy().tobytes() for b in ident.values()]
        before = others()
        got = device_fit_rect(ctx, 0, m, n)
        assert np.array_equal(got["score"], arr["score"])
        assert others() == before
        pairs = device_fit_pairs(ctx, [0, 3, 7], [13, 2, 5])
        assert pairs["score"].tolist() == [arr["score"][0, 13], arr["score"][3, 2], arr["score"][7, 5]]
        assert others() == before
        assert ctx.fit_alignments([(3, 13), (5, 6)]).records["score"].tolist() == [arr["score"][3, 13], arr["score"][5, 6]]
        assert others() == before
        assert np.array_equal(device_fit_rect(ctx, 0, m, n)["db_begin"], arr["db_begin"])


def test_a_strands_context_fits_the_reverse_complements_in_its_later_rows(sa):
    db = make_dna_set(6, 60, 150, 3)
    queries = make_dna_set(4, 20, 70, 4)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rc = [s.translate(comp)[::-1] for s in queries]
    queries[1] = planted(db[2], 10, 40, 5, b"ACGT")
    rc[1] = queries[1].translate(comp)[::-1]
    queries[2] = db[4][30:75].translate(comp)[::-1]  # found on the reverse strand
    rc[2] = db[4][30:75]
    scoring = sa.Scoring.from_names("nw", "nuc44", gap_pen=4)
    n, m = len(db), len(queries)
    ref = [[fit_ref.fit_pair(scoring, d, q) for d in db] for q in queries + rc]
    assert ref[m + 2][4]["db_begin"] == 30 and ref[m + 2][4]["db_end"] == 75 and ref[1][2]["db_begin"] > 0
    with sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0, strands=True) as ctx:
        assert ctx.n_queries == 2 * m
        got = device_fit_rect(ctx, 0, 2 * m, n)
        rev = device_fit_rect(ctx, m, m, n, want=("score", "db_begin", "db_end"))
    for name in OUTPUTS[:5]:
        want = np.array([[r[name] for r in row] for row in ref], np.int64)
        compare(f"strands {name}", got[name], want, db, queries + rc)
        if name in rev:
            assert np.array_equal(rev[name], want[m:])
