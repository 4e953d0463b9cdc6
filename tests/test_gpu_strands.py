"""GPU (-m gpu): both strands of DNA queries, folded on the device (sa_ctx_create_search_strands / sa_ctx_strand_fold /
sa_ctx_hits_strand / sa_ctx_hits_above_strand / sa_hip_search_strands / sa_hip_search_above_strands, csrc/sa_strands.hip).
Contract (include/seqalign_hip.h): a strands context holds the M queries followed by their M reverse complements; cell (q, d) is
reverse iff its reverse value is larger than its forward value, equal values keep the forward strand; hits by folded value
descending, then d ascending; every hit carries the raw score and the strand of the strand that won.

The expectation never comes from the code under test (tests/strands_cases.py): fwd = oracle_rect(db, Q), rev = oracle_rect(db,
rc(Q)) with rc written in Python, strand = rev > fwd, best = where(strand, rev, fwd), hits = expected_hits(best, k).  Under a
quantity both value rectangles are built as tests/test_gpu_search_quantity.py builds its own (NumPy floor division of the oracle's
scores and self-scores; the identity sweep's triangle form, which tests/test_gpu_identity.py pins to the Python restatement), the
fold goes by value and the raw scores are taken at the hits.  Everything is compared exactly.

The conditions that keep an input from passing silently -- both strands among the selected hits, a selected hit that ties between
the strands and is forward, palindrome rows all forward -- are asserted on the expectation before the device is asked, wherever a
shape can hold them: N >= 63 and M >= 3 at k = min(N, 64).  One query has no palindrome beside it, and one hit has one strand.

1. the device-resident chain over the shapes, methods and tables: two ranges, fold out of place and in place, hits, take, strand
2. the asymmetric table and the query lengths of every column class
3. the CSR chain
4. the one-call forms, raw scores and both quantities; batches
5. an index outside [0, N); every refusal of the device-resident calls
6. alignments of the hits on their own strand"""
import numpy as np
import pytest

from tests import tables
from tests.search_cases import expected_hits
from tests.strands_cases import Folded, assert_not_degenerate, dna_database, dna_queries, folded_case, rc
from tests.test_gpu_normalize import INT32_MAX, INT32_MIN, LENGTH, MEAN, MIN, SELF, normalized

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B
NS, MS = (1, 63, 64, 65, 130), (1, 3, 7)
SCORINGS = [(method, matrix) for method in tables.METHODS for matrix in ("nuc44", "dnafull")]
_cases = {}


def scoring_of(sa, method, matrix):
    if matrix == "asym":  # (tests/tables.py: a table that is not symmetric over a lut that holds the whole IUPAC alphabet)
        return tables.scoring_with(sa, method, tables.GAPS[method], tables.asym())
    return sa.Scoring.from_names(method, matrix, **tables.GAPS[method])


def case(sa, oracle, n, m, method, matrix, lengths=None):
    """sequences, stores, scoring and the oracle's expectation (computed once per case)"""
    key = (n, m, method, matrix, lengths)
    if key not in _cases:
        db_seqs = dna_database(n, seed=1000 + n)
        query_seqs = dna_queries(db_seqs, m, seed=2000 + 10 * n + m, lengths=lengths)
        scoring = scoring_of(sa, method, matrix)
        exp = folded_case(sa, oracle, db_seqs, query_seqs, scoring)
        for a in (exp.fwd, exp.rev, exp.strand, exp.best):
            a.setflags(write=False)
        _cases[key] = (tables.raw_store(sa, db_seqs), tables.raw_store(sa, query_seqs), scoring, exp, db_seqs, query_seqs)
    return _cases[key]


def ks_of(n):
    return sorted({1, min(n, 64)})


def palindromes_of(m, lengths=None):
    return 2 if m >= 3 and lengths is None else 0


class Dev:
    """device buffers with a poisoned tail each: what is written beyond the contract's size is seen"""
    TAIL = 64

    def __init__(self, torch):
        self.torch, self.sizes, self.bufs = torch, {}, {}

    def new(self, name, elems, dtype, fill=None):
        t = self.torch
        poison = {t.int32: POISON, t.int64: 0x5A5A5A5A5A5A5A5A, t.uint8: 0x5A}[dtype]
        self.bufs[name] = t.full((elems + self.TAIL,), poison, dtype=dtype, device="cuda")
        self.sizes[name] = elems
        if fill is not None:
            self.bufs[name][:elems] = t.from_numpy(np.array(fill).reshape(-1)).cuda()
        return self.bufs[name].data_ptr()

    def get(self, name, shape=None):
        host = self.bufs[name].cpu().numpy()
        n = self.sizes[name]
        poison = {np.dtype(np.int32): POISON, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A, np.dtype(np.uint8): 0x5A}[host.dtype]
        assert (host[n:] == poison).all(), f"{name}: written beyond its {n} elements"
        return host[:n] if shape is None else host[:n].reshape(shape)


def device_ranges(torch, ctx, dev, n, m):
    """the two halves of the rows through the existing call: d_fwd, d_rev"""
    pf, pr = dev.new("fwd", m * n, torch.int32), dev.new("rev", m * n, torch.int32)
    scratch = torch.empty(max(ctx.search_scratch_bytes(m, m) // 4, 1), dtype=torch.int32, device="cuda")
    assert ctx.search_scratch_bytes(m, m) >= ctx.search_scratch_bytes(0, m)
    ctx.search_range(0, m, pf, scratch.data_ptr())
    ctx.search_range(m, m, pr, scratch.data_ptr())
    torch.cuda.synchronize()
    return pf, pr


def bits_u64(a):
    return a.view(np.uint64) if a.dtype == np.int64 else a


def check_chain(sa, torch, ctx, exp, what):
    """fold out of place and in place (raw scores, then LENGTH-style values with the raw scores carried), hits, take, strand"""
    n, m = exp.n, exp.m
    words = sa.strand_words(n)
    dev = Dev(torch)
    pf, pr = device_ranges(torch, ctx, dev, n, m)
    assert np.array_equal(dev.get("fwd", (m, n)), exp.fwd), f"{what}: the forward rows"
    assert np.array_equal(dev.get("rev", (m, n)), exp.rev), f"{what}: the rows M + q are the reverse complements"
    # raw scores: value is score, out of place
    pb, pbits = dev.new("best", m * n, torch.int32), dev.new("bits", m * words, torch.int64)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.strand_fold(pf, pr, m, pb, pbits, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(dev.get("best", (m, n)), exp.best), f"{what}: folded scores"
    assert np.array_equal(bits_u64(dev.get("bits", (m, words))), exp.bits()), f"{what}: bitmap (tail bits zero)"
    assert np.array_equal(dev.get("fwd", (m, n)), exp.fwd) and np.array_equal(dev.get("rev", (m, n)), exp.rev), f"{what}: the inputs changed"
    # values that differ from the scores (NumPy's own division by the lengths of the test's choosing), the scores carried along
    den_d, den_q = 50 + np.arange(n) % 37, 40 + np.arange(m) % 11
    vexp = Folded(exp.fwd, exp.rev, normalized(exp.fwd, den_d[None, :], den_q[:, None], MIN), normalized(exp.rev, den_d[None, :], den_q[:, None], MIN))
    pvf, pvr = dev.new("vfwd", m * n, torch.int32, vexp.vfwd), dev.new("vrev", m * n, torch.int32, vexp.vrev)
    pvb, psb, pvbits = dev.new("vbest", m * n, torch.int32), dev.new("sbest", m * n, torch.int32), dev.new("vbits", m * words, torch.int64)
    torch.cuda.synchronize()
    ctx.strand_fold(pvf, pvr, m, pvb, pvbits, d_sfwd_ptr=pf, d_srev_ptr=pr, d_sbest_ptr=psb, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(dev.get("vbest", (m, n)), vexp.vbest) and np.array_equal(dev.get("sbest", (m, n)), vexp.best), f"{what}: fold by value"
    assert np.array_equal(bits_u64(dev.get("vbits", (m, words))), vexp.bits()), f"{what}: bitmap by value"
    # in place: vbest = vfwd, sbest = sfwd, no bitmap; then raw in place with one
    pf2 = dev.new("fwd2", m * n, torch.int32, exp.fwd)
    torch.cuda.synchronize()
    ctx.strand_fold(pvf, pvr, m, pvf, 0, d_sfwd_ptr=pf2, d_srev_ptr=pr, d_sbest_ptr=pf2, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(dev.get("vfwd", (m, n)), vexp.vbest) and np.array_equal(dev.get("fwd2", (m, n)), vexp.best), f"{what}: in place by value"
    assert np.array_equal(dev.get("vrev", (m, n)), vexp.vrev) and np.array_equal(dev.get("rev", (m, n)), exp.rev)
    dev.new("bits", m * words, torch.int64)
    ctx.strand_fold(pf, pr, m, pf, dev.bufs["bits"].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(dev.get("fwd", (m, n)), exp.best), f"{what}: in place"
    assert np.array_equal(bits_u64(dev.get("bits", (m, words))), exp.bits()), f"{what}: bitmap in place"
    pbits = dev.bufs["bits"].data_ptr()
    for k in ks_of(n):
        wi, wv, ws, wst = exp.hits(k)
        pi, pv, ps, pst = (dev.new(name, m * k, dt) for name, dt in (("index", torch.int32), ("value", torch.int32), ("score", torch.int32),
                                                                     ("strand", torch.uint8)))
        part = torch.empty(max(sa.hits_scratch_bytes(n, m, k) // 8, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.hits(pf, m, k, pi, pv, part.data_ptr(), stream=stream.cuda_stream)
        ctx.hits_take(pf, m, k, pi, ps, stream=stream.cuda_stream)
        ctx.hits_strand(pbits, m, k, pi, pst, stream=stream.cuda_stream)
        stream.synchronize()
        for name, want in (("index", wi), ("value", wv), ("score", ws), ("strand", wst)):
            got = dev.get(name, (m, k))
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{what} k={k} {name}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


# ---- 1. the chain over the shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,matrix", SCORINGS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_device_resident_chain(n, m, method, matrix, sa, oracle):
    import torch
    db, queries, scoring, exp, *_ = case(sa, oracle, n, m, method, matrix)
    what = f"{method} {matrix} ({n}, {m})"
    if n >= 63 and m >= 3:
        assert_not_degenerate(exp, min(n, 64), palindromes_of(m), what)
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx:
        assert (ctx.n_db, ctx.n_queries, ctx.strands, ctx.n_strand_queries) == (n, 2 * m, 2, m)
        check_chain(sa, torch, ctx, exp, what)


def test_plain_contexts_answer_one_and_zero(sa, oracle):
    db, queries, scoring, *_ = case(sa, oracle, 63, 3, "sw", "nuc44")
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        assert (ctx.strands, ctx.n_queries, ctx.n_strand_queries) == (1, 3, 3)
    with sa.Context(db, scoring, 0) as plain:
        assert sa.load_library().sa_ctx_search_strands(plain._h) == 0


# ---- 2. the asymmetric table; every column class ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", tables.METHODS)
def test_asymmetric_table(method, sa, oracle):
    """the search of rc(Q) is no mirror of the search of Q under a table that is not symmetric: both rows come from the oracle"""
    import torch
    n, m = 65, 7
    db, queries, scoring, exp, *_ = case(sa, oracle, n, m, method, "asym")
    assert_not_degenerate(exp, 64, 2, f"{method} asym")
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx:
        check_chain(sa, torch, ctx, exp, f"{method} asym")


LENGTHS = (5, 64, 65, 129, 300, 1025)


def test_reverse_rows_in_every_column_class(sa, oracle):
    import torch
    n, m = 65, len(LENGTHS)
    db, queries, scoring, exp, _, query_seqs = case(sa, oracle, n, m, "sw", "nuc44", lengths=LENGTHS)
    assert tuple(len(q) for q in query_seqs) == LENGTHS
    index, _, _, strand = exp.hits(64)
    assert (strand == 0).any() and (strand == 1).any()
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx:
        check_chain(sa, torch, ctx, exp, "column classes")


# ---- 3. the CSR chain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (65, 3), (130, 7)])
def test_csr_chain(n, m, sa, oracle):
    import torch
    db, queries, scoring, exp, *_ = case(sa, oracle, n, m, "sw", "nuc44")
    words = sa.strand_words(n)
    middle = int(np.sort(exp.best.reshape(-1))[exp.best.size // 2])
    above = int(exp.best.max()) + 1
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx:
        dev = Dev(torch)
        pf, pr = device_ranges(torch, ctx, dev, n, m)
        pbits = dev.new("bits", m * words, torch.int64)
        ctx.strand_fold(pf, pr, m, pf, pbits)
        torch.cuda.synchronize()
        for t in (INT32_MIN, middle, above):
            woff, wi, wv, ws, wst = exp.above(t)
            e = int(woff[-1])
            assert e == {INT32_MIN: m * n, above: 0}.get(t, e) and (t != middle or 0 < e < m * n or m * n == 1)
            poff = dev.new("offsets", m + 1, torch.int64)
            scratch = torch.empty(sa.hits_above_scratch_bytes(n, m) // 8, dtype=torch.int64, device="cuda")
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            ctx.hits_above_offsets(pf, m, t, poff, scratch.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(dev.get("offsets"), woff), f"threshold {t}: offsets"
            pi, pv, pst = dev.new("index", e, torch.int32), dev.new("value", e, torch.int32), dev.new("strand", e, torch.uint8)
            torch.cuda.synchronize()
            ctx.hits_above_fill(pf, pf, m, t, poff, scratch.data_ptr(), pi, pv, stream=stream.cuda_stream)
            ctx.hits_above_strand(pbits, m, poff, pi, pst, stream=stream.cuda_stream)  # (the empty result must be valid)
            stream.synchronize()
            assert np.array_equal(dev.get("index"), wi) and np.array_equal(dev.get("value"), wv), f"threshold {t}: fill"
            assert np.array_equal(dev.get("strand"), wst), f"threshold {t}: strands of the entries"
            if t == middle and n >= 65:
                assert (wst == 0).any() and (wst == 1).any()


# ---- 4. the one-call forms ----------------------------------------------------------------------------------------------------------------
def quantity_case(sa, oracle, kind):
    """(keyword arguments, expectation, denominators or None) of the (130, 7) SW case under a quantity"""
    db, queries, scoring, exp, db_seqs, query_seqs = case(sa, oracle, 130, 7, "sw", "nuc44")
    n, m = exp.n, exp.m
    key = ("quantity", kind)
    if key not in _cases:
        rows = list(query_seqs) + [rc(q) for q in query_seqs]
        if kind == ("raw",):
            _cases[key] = ({}, exp, None)
        elif kind[0] == "norm":
            _, source, rule = kind
            den = np.array([len(s) for s in db_seqs + rows] if source == LENGTH else [oracle.pair(scoring, s, s) for s in db_seqs + rows], np.int32)
            vf = normalized(exp.fwd, den[None, :n], den[n:n + m, None], rule)
            vr = normalized(exp.rev, den[None, :n], den[n + m:, None], rule)
            _cases[key] = (dict(norm=sa.Norm(source, rule)), Folded(exp.fwd, exp.rev, vf, vr), den)
        else:  # percent identity: the triangle form of the sweep over db, Q, rc(Q), gathered at tri(N + row) + d
            cat = sa.SequenceStore.from_sequences(list(db_seqs) + rows)
            at = np.array([[(n + q) * (n + q - 1) // 2 + d for d in range(n)] for q in range(2 * m)], np.int64)
            pid = np.ascontiguousarray(sa.hip_identity(cat, scoring, denom=kind[1], identities=False, columns=False)[2][at])
            _cases[key] = (dict(pid=kind[1]), Folded(exp.fwd, exp.rev, pid[:m], pid[m:]), None)
    return (db, queries, scoring) + _cases[key]


KINDS = [("raw",), ("norm", SELF, MEAN), ("norm", LENGTH, MIN), ("pid", 1), ("pid", 0)]


def check_one_call(got, exp, den, k, what):
    index, value, score, strand, rect, vrect, srect = got[:7]
    assert np.array_equal(rect, exp.best), f"{what}: folded rect"
    assert np.array_equal(vrect, exp.vbest), f"{what}: folded vrect"
    assert srect.dtype == np.uint8 and np.array_equal(srect, exp.strand.astype(np.uint8)), f"{what}: srect"
    for name, g, w in zip(("index", "value", "score", "strand"), (index, value, score, strand), exp.hits(k)):
        assert g.dtype == w.dtype and g.shape == (exp.m, k) and np.array_equal(g, w), f"{what} k={k} {name}"
    if den is not None:
        assert len(got) == 8 and np.array_equal(got[7], den), f"{what}: the N + 2 M denominators"
    else:
        assert len(got) == 7


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "-".join(map(str, k)))
def test_one_call(kind, sa, oracle):
    db, queries, scoring, kw, exp, den = quantity_case(sa, oracle, kind)
    assert_not_degenerate(exp, 64, 2, str(kind))
    if kind != ("raw",):
        raw = case(sa, oracle, 130, 7, "sw", "nuc44")[3]
        assert (exp.strand != raw.strand).any() or not np.array_equal(exp.hits(64)[0], raw.hits(64)[0]), "by value the answer is the raw one: the case shows nothing"
    for k in (1, 64):
        check_one_call(sa.hip_search_strands(db, queries, scoring, k=k, rect=True, **kw), exp, den, k, str(kind))
    assert sa.last_search_strands_seconds() > 0 and sa.last_search_breakdown()["batches"] == 1
    assert (sa.last_search_quantity_seconds() > 0) == (kind != ("raw",))
    # the hits alone, the rectangles alone
    alone = sa.hip_search_strands(db, queries, scoring, k=7, **kw)
    assert all(np.array_equal(g, w) for g, w in zip(alone[:4], exp.hits(7)))
    rects = sa.hip_search_strands(db, queries, scoring, rect=True, **kw)
    assert np.array_equal(rects[0], exp.best) and np.array_equal(rects[1], exp.vbest) and np.array_equal(rects[2], exp.strand.astype(np.uint8))


@pytest.mark.parametrize("kind", [("raw",), ("norm", SELF, MEAN), ("pid", 1)], ids=lambda k: "-".join(map(str, k)))
def test_one_call_above(kind, sa, oracle):
    db, queries, scoring, kw, exp, den = quantity_case(sa, oracle, kind)
    middle = int(np.sort(exp.vbest.reshape(-1))[exp.vbest.size * 3 // 4])
    for t in (INT32_MIN, middle, int(exp.vbest.max()) + 1):
        woff, wi, wv, ws, wst = exp.above(t)
        got = sa.hip_search_above_strands(db, queries, scoring, t, **kw)
        assert np.array_equal(got.offsets, woff) and np.array_equal(got.index, wi), f"{kind} threshold {t}"
        assert np.array_equal(got.value, wv) and np.array_equal(got.score, ws), f"{kind} threshold {t}: value / score"
        assert got.strand is not None and got.strand.dtype == np.uint8 and np.array_equal(got.strand, wst), f"{kind} threshold {t}: strand"
        if den is not None:
            assert np.array_equal(got.denominators, den)
    assert 0 < len(exp.above(middle)[1]) < exp.m * exp.n and {0, 1} <= set(exp.above(middle)[4].tolist())
    assert sa.last_search_strands_seconds() > 0
    assert sa.hip_search_above(db, queries, scoring, middle).strand is None


@pytest.mark.parametrize("kind", [("raw",), ("norm", SELF, MEAN), ("pid", 1)], ids=lambda k: "-".join(map(str, k)))
def test_batches_give_the_bytes_of_the_unbatched_expectation(kind, sa, oracle, monkeypatch):
    db, queries, scoring, kw, exp, den = quantity_case(sa, oracle, kind)
    n, m, k = exp.n, exp.m, 64
    words = sa.strand_words(n)
    # (include/seqalign_hip.h: sa_hip_search_strands)
    per_query = (0 if kind[0] == "pid" else 4 * (n + 2 * m)) + (8 if kind == ("raw",) else 16) * n + 8 * words + 21 * k
    monkeypatch.setenv("SA_HIP_SEARCH_BATCH_BYTES", str(2 * per_query))  # two queries a batch: four batches
    check_one_call(sa.hip_search_strands(db, queries, scoring, k=k, rect=True, **kw), exp, den, k, f"{kind} in batches")
    assert sa.last_search_breakdown()["batches"] == 4
    per_query = (0 if kind[0] == "pid" else 4 * (n + 2 * m)) + (8 if kind == ("raw",) else 16) * n + 8 * words + 8
    monkeypatch.setenv("SA_HIP_SEARCH_BATCH_BYTES", str(3 * per_query))  # three queries a batch: three batches
    t = int(np.sort(exp.vbest.reshape(-1))[exp.vbest.size // 2])
    woff, wi, wv, ws, wst = exp.above(t)
    got = sa.hip_search_above_strands(db, queries, scoring, t, **kw)
    assert sa.last_search_breakdown()["batches"] == 3
    for g, w in zip((got.offsets, got.index, got.value, got.score, got.strand), (woff, wi, wv, ws, wst)):
        assert np.array_equal(g, w)


# ---- 5. an index outside [0, N); refusals ---------------------------------------------------------------------------------------------
def test_index_out_of_range_gives_255(sa, oracle):
    import torch
    n, m, k = 65, 3, 4
    db, queries, scoring, exp, *_ = case(sa, oracle, n, m, "sw", "nuc44")
    bits = exp.bits()
    index = np.array([[0, -1, 64, 65], [INT32_MIN, INT32_MAX, 63, 1], [n, n - 1, -2**20, 2]], np.int32)
    want = np.array([[exp.strand[r, d] if 0 <= d < n else 255 for d in row] for r, row in enumerate(index)], np.uint8)
    assert (want == 255).sum() == 6 and sa.STRAND_NONE == 255
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx:
        dev = Dev(torch)
        pbits, pi, pst = dev.new("bits", bits.size, torch.int64, bits.view(np.int64)), dev.new("index", m * k, torch.int32, index), dev.new("strand", m * k, torch.uint8)
        torch.cuda.synchronize()
        ctx.hits_strand(pbits, m, k, pi, pst)
        torch.cuda.synchronize()
        assert np.array_equal(dev.get("strand", (m, k)), want)
        # ... and over a CSR whose entries are these rows
        poff, pcs = dev.new("offsets", m + 1, torch.int64, np.arange(m + 1, dtype=np.int64) * k), dev.new("cstrand", m * k, torch.uint8)
        torch.cuda.synchronize()
        ctx.hits_above_strand(pbits, m, poff, pi, pcs)
        torch.cuda.synchronize()
        assert np.array_equal(dev.get("cstrand", (m, k)), want)


def test_refusals_of_the_device_resident_calls(sa, oracle):
    """every refusal with its message, nothing launched (the poison stays), each followed by a valid call"""
    import torch
    n, m, k = 65, 3, 2
    db, queries, scoring, exp, *_ = case(sa, oracle, n, m, "sw", "nuc44")
    words = sa.strand_words(n)
    wi = exp.hits(k)[0]
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx, sa.SearchContext(db, queries, scoring, 0) as single, \
            sa.Context(db, scoring, 0) as plain:
        dev = Dev(torch)
        f, r = dev.new("fwd", m * n, torch.int32, exp.fwd), dev.new("rev", m * n, torch.int32, exp.rev)
        out = dev.new("out", m * n + 2, torch.int32)
        bits = dev.new("bits", m * words + 1, torch.int64)
        good = dev.new("good", m * words, torch.int64, exp.bits().view(np.int64))
        x = dev.new("index", m * k + 1, torch.int32, np.concatenate([wi.reshape(-1), [0]]))
        off = dev.new("offsets", m + 2, torch.int64, np.concatenate([np.arange(m + 1) * k, [0]]))
        st = dev.new("strand", m * k, torch.uint8)
        torch.cuda.synchronize()

        def untouched():
            torch.cuda.synchronize()
            for name in ("out", "bits", "strand"):
                got = dev.bufs[name].cpu().numpy()
                assert (got == {np.dtype(np.int32): POISON, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A, np.dtype(np.uint8): 0x5A}[got.dtype]).all(), name

        def valid():
            ctx.strand_fold(f, r, m, out, bits)
            ctx.hits_strand(good, m, k, x, st)
            torch.cuda.synchronize()
            assert np.array_equal(dev.bufs["out"].cpu().numpy()[:m * n].reshape(m, n), exp.best)
            assert np.array_equal(dev.bufs["strand"].cpu().numpy()[:m * k].reshape(m, k), exp.hits(k)[3])
            ctx.hits_above_strand(good, m, off, x, st)
            torch.cuda.synchronize()
            assert np.array_equal(dev.bufs["strand"].cpu().numpy()[:m * k].reshape(m, k), exp.hits(k)[3])
            for name, dt in (("out", torch.int32), ("bits", torch.int64), ("strand", torch.uint8)):
                dev.bufs[name].fill_({torch.int32: POISON, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A}[dt])
            torch.cuda.synchronize()

        SC = sa.SearchContext
        refusals = [
            ("sa_ctx_strand_fold: not a strands context", lambda: SC.strand_fold(single, f, r, m, out, bits)),
            ("sa_ctx_strand_fold: not a search context", lambda: SC.strand_fold(plain, f, r, m, out, bits)),
            ("sa_ctx_strand_fold: null argument", lambda: ctx.strand_fold(0, r, m, out, bits)),
            ("sa_ctx_strand_fold: null argument", lambda: ctx.strand_fold(f, 0, m, out, bits)),
            ("sa_ctx_strand_fold: null argument", lambda: ctx.strand_fold(f, r, m, 0, bits)),
            (r"sa_ctx_strand_fold: 0 rows, .* nq must be in \[1, 3\]", lambda: ctx.strand_fold(f, r, 0, out, bits)),
            (r"sa_ctx_strand_fold: 4 rows, .* nq must be in \[1, 3\]", lambda: ctx.strand_fold(f, r, m + 1, out, bits)),
            (r"sa_ctx_strand_fold: 6 rows", lambda: ctx.strand_fold(f, r, 2 * m, out, bits)),  # (2 M rows the context has; M queries)
            ("sa_ctx_strand_fold: d_bits not 8-byte aligned", lambda: ctx.strand_fold(f, r, m, out, bits + 4)),
            ("sa_ctx_strand_fold: the rectangles want 4-byte alignment", lambda: ctx.strand_fold(f + 2, r, m, out, bits)),
            ("sa_ctx_strand_fold: the rectangles want 4-byte alignment", lambda: ctx.strand_fold(f, r + 1, m, out, bits)),
            ("sa_ctx_strand_fold: the rectangles want 4-byte alignment", lambda: ctx.strand_fold(f, r, m, out + 3, bits)),
            ("all three or none", lambda: ctx.strand_fold(f, r, m, out, bits, d_sfwd_ptr=f)),
            ("all three or none", lambda: ctx.strand_fold(f, r, m, out, bits, d_sfwd_ptr=f, d_srev_ptr=r)),
            ("all three or none", lambda: ctx.strand_fold(f, r, m, out, bits, d_sbest_ptr=out)),
            ("sa_ctx_strand_fold: the rectangles want 4-byte alignment", lambda: ctx.strand_fold(f, r, m, out, bits, d_sfwd_ptr=f, d_srev_ptr=r + 2, d_sbest_ptr=out)),
            ("sa_ctx_hits_strand: not a strands context", lambda: SC.hits_strand(single, good, m, k, x, st)),
            ("sa_ctx_hits_strand: not a search context", lambda: SC.hits_strand(plain, good, m, k, x, st)),
            ("sa_ctx_hits_strand: null argument", lambda: ctx.hits_strand(0, m, k, x, st)),
            ("sa_ctx_hits_strand: null argument", lambda: ctx.hits_strand(good, m, k, 0, st)),
            ("sa_ctx_hits_strand: null argument", lambda: ctx.hits_strand(good, m, k, x, 0)),
            (r"sa_ctx_hits_strand: 0 rows", lambda: ctx.hits_strand(good, 0, k, x, st)),
            (r"sa_ctx_hits_strand: 4 rows", lambda: ctx.hits_strand(good, m + 1, k, x, st)),
            ("sa_ctx_hits_strand: k = 0 hits", lambda: ctx.hits_strand(good, m, 0, x, st)),
            ("sa_ctx_hits_strand: k = 65 hits", lambda: ctx.hits_strand(good, m, 65, x, st)),
            ("sa_ctx_hits_strand: d_bits not 8-byte aligned", lambda: ctx.hits_strand(good + 4, m, k, x, st)),
            ("sa_ctx_hits_strand: d_index wants 4-byte alignment", lambda: ctx.hits_strand(good, m, k, x + 2, st)),
            ("sa_ctx_hits_above_strand: not a strands context", lambda: SC.hits_above_strand(single, good, m, off, x, st)),
            ("sa_ctx_hits_above_strand: not a search context", lambda: SC.hits_above_strand(plain, good, m, off, x, st)),
            ("sa_ctx_hits_above_strand: null argument", lambda: ctx.hits_above_strand(0, m, off, x, st)),
            ("sa_ctx_hits_above_strand: null argument", lambda: ctx.hits_above_strand(good, m, 0, x, st)),
            ("sa_ctx_hits_above_strand: null argument", lambda: ctx.hits_above_strand(good, m, off, 0, st)),
            ("sa_ctx_hits_above_strand: null argument", lambda: ctx.hits_above_strand(good, m, off, x, 0)),
            (r"sa_ctx_hits_above_strand: 0 rows", lambda: ctx.hits_above_strand(good, 0, off, x, st)),
            (r"sa_ctx_hits_above_strand: 4 rows", lambda: ctx.hits_above_strand(good, m + 1, off, x, st)),
            ("sa_ctx_hits_above_strand: d_bits not 8-byte aligned", lambda: ctx.hits_above_strand(good + 2, m, off, x, st)),
            ("sa_ctx_hits_above_strand: d_offsets wants 8-byte", lambda: ctx.hits_above_strand(good, m, off + 4, x, st)),
            ("sa_ctx_hits_above_strand: d_offsets wants 8-byte", lambda: ctx.hits_above_strand(good, m, off, x + 1, st)),
        ]
        for message, call in refusals:
            with pytest.raises(sa.AlignError, match=message):
                call()
            untouched()
            valid()
        # rectangles at 4-byte alignment and no more are accepted: views one element off
        ctx.strand_fold(f, r, m, out + 4, bits)
        torch.cuda.synchronize()
        assert np.array_equal(dev.bufs["out"].cpu().numpy()[1:m * n + 1].reshape(m, n), exp.best)


def test_creation_refuses_what_cannot_be_complemented(sa, oracle):
    db, queries, scoring, *_ = case(sa, oracle, 63, 3, "sw", "nuc44")
    bad = tables.raw_store(sa, [b"ACGT", b"ACGTXA", b"AC"])
    with pytest.raises(sa.AlignError, match=r"sa_ctx_create_search_strands: sequence #2 .* residue 5 is byte 0x58 \('X'\)"):
        sa.SearchContext(db, bad, scoring, 0, strands=True)
    comp = sa.dna_complement()
    comp[ord("A")] = ord("J")  # a table of the caller's whose complement the scoring's alphabet does not hold
    with pytest.raises(sa.AlignError, match=r"sequence #1 .* residue 1 is byte 0x41 \('A'\), whose complement 'J'"):
        sa.SearchContext(db, tables.raw_store(sa, [b"ACGT"]), scoring, 0, strands=True, comp=comp)


# ---- 6. alignments of the hits ------------------------------------------------------------------------------------------------------------
def test_alignments_of_every_hit_on_its_own_strand(sa, oracle):
    n, m, k = 130, 7, 9
    db, queries, scoring, exp, _, query_seqs = case(sa, oracle, n, m, "sw", "nuc44")
    index, _, score, strand = exp.hits(k)
    assert (strand == 0).any() and (strand == 1).any()
    with sa.SearchContext(db, queries, scoring, 0, strands=True) as ctx:
        pairs = [(n + int(strand[q, t]) * m + q, int(index[q, t])) for q in range(m) for t in range(k)]
        alns = ctx.alignments(pairs)
        got = alns.records["score"].reshape(m, k)
        assert np.array_equal(got, score), "the alignment of a hit on its strand's row scores rect[q, d]"
        assert np.array_equal(got, np.take_along_axis(exp.best, index.astype(np.int64), 1))
        # on the other strand's row the score is the other rectangle's
        other = ctx.alignments([(n + (1 - int(strand[q, t])) * m + q, int(index[q, t])) for q in range(m) for t in range(k)])
        want = np.take_along_axis(np.where(exp.strand, exp.fwd, exp.rev), index.astype(np.int64), 1)
        assert np.array_equal(other.records["score"].reshape(m, k), want)
        # the a_* span of a reverse hit refers to the reverse complement of the query
        t = int(np.flatnonzero(strand.reshape(-1) == 1)[0])
        q = t // k
        a_begin, a_end = int(alns.records["a_begin"][t]), int(alns.records["a_end"][t])
        assert 0 <= a_begin <= a_end <= len(query_seqs[q])
