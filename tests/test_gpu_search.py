"""GPU (-m gpu): queries against a database (sa_ctx_create_search / sa_ctx_search_range / sa_ctx_hits / sa_hip_search,
csrc/sa_search.hip; the row bound of the planner and of the systolic kernels).  Contract (include/seqalign_hip.h): the score of
query q against database sequence d is pair (d, N + q) of the concatenated store; rect[q, d]; the hits of q are all d by score
descending, then d ascending.

The expectation never comes from the code under test: rect = rows N.., columns ..N of tri_to_full(oracle.align(concatenated
store)), hits = np.lexsort((d, -scores))[:k] per row of that.  Everything is compared exactly."""
import numpy as np
import pytest

from tests import tables
from tests.search_cases import MIXED_QUERY_LENGTHS, expected_hits, oracle_rect
from tests.synth import make_dna_set, make_protein_set

pytestmark = pytest.mark.gpu

GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}
POISON = -0x5A5A5A5B


def assert_same_hits(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == np.int32 and gs.dtype == np.int32 and gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.argwhere((gi != wi) | (gs != ws))
    assert bad.size == 0, (f"{what}: {len(bad)} entries differ, first at row {bad[0][0]} place {bad[0][1]}: "
                           f"got ({gi[tuple(bad[0])]}, {gs[tuple(bad[0])]}), want ({wi[tuple(bad[0])]}, {ws[tuple(bad[0])]})")


_cache = {}


def protein_case(sa, oracle, method: str, n: int, m: int):
    """db, queries, scoring and the oracle's rectangle of N + M short proteins (computed once per method and shape)"""
    key = (method, n, m)
    if key not in _cache:
        db_seqs, query_seqs = make_protein_set(n, 20, 60, 11), make_protein_set(m, 20, 60, 12)
        scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
        want = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
        want.setflags(write=False)
        _cache[key] = (sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring, want, db_seqs, query_seqs)
    return _cache[key]


# ---- 1. the rectangle against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (3, 5), (40, 130), (700, 65)])
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_rect_equals_the_oracle(method, n, m, sa, oracle):
    db, queries, scoring, want, *_ = protein_case(sa, oracle, method, n, m)
    got = sa.hip_search(db, queries, scoring, rect=True)
    assert got.dtype == np.int32 and got.shape == (m, n)
    assert np.array_equal(got, want), f"{method} ({n}, {m}): {np.count_nonzero(got != want)} of {want.size} differ"


def test_rect_of_mixed_column_lengths(sa, oracle):
    """8-lane, 16-lane, s32 and strip-mined query columns over one database, nw"""
    db_seqs = make_protein_set(300, 20, 60, 11)
    query_seqs = [make_protein_set(1, ln, ln, 100 + t)[0] for t, ln in enumerate(MIXED_QUERY_LENGTHS)]
    scoring = sa.Scoring.from_names("nw", "blosum62", **GAPS["nw"])
    want = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
    got = sa.hip_search(sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring, rect=True)
    assert np.array_equal(got, want), f"rows that differ: {sorted(set(np.argwhere(got != want)[:, 0].tolist()))}"


@pytest.mark.parametrize("switch", ["SA_HIP_FORCE_GENERIC", "SA_HIP_NO_PK"])
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_rect_on_the_other_kernel_families(method, switch, sa, oracle, monkeypatch):
    db, queries, scoring, want, *_ = protein_case(sa, oracle, method, 700, 65)
    monkeypatch.setenv(switch, "1")  # (read when the context is created)
    assert np.array_equal(sa.hip_search(db, queries, scoring, rect=True), want), f"{method} under {switch}"


# ---- 2. asymmetric table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_asymmetric_table_keeps_its_orientation(method, sa, oracle):
    n, m = 65, 20
    db_seqs = tables.random_sequences([30 + (7 * t) % 31 for t in range(n)], seed=21)
    query_seqs = tables.random_sequences([25 + (5 * t) % 29 for t in range(m)], seed=22)
    scoring = tables.scoring_with(sa, method, GAPS[method], tables.asym())
    want = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
    other = oracle_rect(sa, oracle, db_seqs, query_seqs, tables.transposed(scoring))
    differ = int(np.count_nonzero(want != other))
    print(f"{method}: {differ} of {want.size} entries differ between the table and its transpose (oracle)")
    assert differ >= 10  # from the oracle alone, before the device is asked: the case does test the orientation
    got = sa.hip_search(tables.raw_store(sa, db_seqs), tables.raw_store(sa, query_seqs), scoring, rect=True)
    assert np.array_equal(got, want), f"{method}: {np.count_nonzero(got != want)} differ; {np.count_nonzero(got != other)} from the transposed table's"


# ---- 3. device-resident -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q0,nq", [(0, 65), (17, 1), (62, 3)])
def test_search_range_on_a_stream_writes_nothing_else(q0, nq, sa, oracle):
    import torch
    n, m = 700, 65
    db, queries, scoring, want, *_ = protein_case(sa, oracle, "ga", n, m)
    tail = 4096
    d_rect = torch.full((nq * n + tail,), POISON, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        assert (ctx.n_db, ctx.n_queries) == (n, m)
        need = ctx.search_scratch_bytes(q0, nq)
        assert need == 4 * sum(n + q for q in range(q0, q0 + nq))
        d_scratch = torch.full((need // 4 + tail,), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.search_range(q0, nq, d_rect.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        for bad in ((-1, 1), (m, 1), (q0, m - q0 + 1), (0, 0)):
            with pytest.raises(sa.AlignError, match="queries"):
                ctx.search_range(*bad, d_rect.data_ptr(), d_scratch.data_ptr())
    rect, scratch = d_rect.cpu().numpy(), d_scratch.cpu().numpy()
    assert (rect[nq * n:] == POISON).all() and (scratch[need // 4:] == POISON).all(), "written beyond the rectangle or the scratch"
    assert np.array_equal(rect[:nq * n].reshape(nq, n), want[q0:q0 + nq])


def test_no_query_query_pair_is_computed(sa, oracle):
    """queries of one length fall into one kernel: its pair count is nq * N exactly"""
    import torch
    n, m = 700, 65
    db_seqs = make_protein_set(n, 20, 60, 11)
    query_seqs = make_protein_set(m, 44, 44, 13)
    scoring = sa.Scoring.from_names("nw", "blosum62", **GAPS["nw"])
    want = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
    with sa.SearchContext(sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring, 0) as ctx:
        for q0, nq in ((0, m), (17, 1), (m - 3, 3)):
            d_rect = torch.empty(nq * n, dtype=torch.int32, device="cuda")
            d_scratch = torch.empty(ctx.search_scratch_bytes(q0, nq) // 4, dtype=torch.int32, device="cuda")
            ctx.timing(True)
            ctx.search_range(q0, nq, d_rect.data_ptr(), d_scratch.data_ptr())
            torch.cuda.synchronize()
            t = ctx.timing_read()
            ctx.timing(False)
            assert t["pairs"] == nq * n and t["launches"] == 1, t
            assert np.array_equal(d_rect.cpu().numpy().reshape(nq, n), want[q0:q0 + nq])


def test_a_search_context_refuses_the_packed_calls(sa, oracle):
    import torch
    db, queries, scoring, *_ = protein_case(sa, oracle, "nw", 40, 130)
    d = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    p = d.data_ptr()
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        calls = [lambda: ctx.align_range(0, 16, p), lambda: ctx.align_range16(0, 16, p), lambda: ctx.align_host(None, True),
                 lambda: ctx.share_elems(0, 16, 1), lambda: ctx.align_share(0, 16, 1, 0, p, False), lambda: ctx.place_shares(0, 16, 1, p, False, p),
                 lambda: ctx.expand_full(p, p), lambda: ctx.neighbors(p, 1, p, p), lambda: ctx.edge_offsets(p, 0, p),
                 lambda: ctx.edge_fill(p, 0, p, p, p), lambda: ctx.linkage(p, p, p, p), lambda: ctx.agglomerate(p, sa.AGGLO_COMPLETE, p, p, p),
                 lambda: ctx.select(p, [0], p, p, p), lambda: ctx.normalize(p, p, sa.NORM_MIN, p), lambda: ctx.identity_range(0, 16, score=p)]
        for call in calls:
            with pytest.raises(sa.AlignError, match="sa_ctx_search_range"):
                call()
        assert ctx.token_tiles() is not None
    with sa.Context(db, scoring, 0) as plain:  # ... and an ordinary context refuses the search calls
        with pytest.raises(sa.AlignError, match="not a search context"):
            sa.SearchContext.search_range(plain, 0, 1, p, p)
        with pytest.raises(sa.AlignError, match="not a search context"):
            sa.SearchContext.hits(plain, p, 1, 1, p, p)
        assert plain._lib.sa_ctx_search_db(plain._h) == 0 and plain._lib.sa_ctx_search_queries(plain._h) == 0


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------
def test_batches_give_the_same_bytes(sa, oracle, monkeypatch):
    n, m, k = 700, 65, 7
    db, queries, scoring, want, *_ = protein_case(sa, oracle, "sw", n, m)
    one = sa.hip_search(db, queries, scoring, k=k, rect=True)
    assert sa.last_search_breakdown()["batches"] == 1
    monkeypatch.setenv("SA_HIP_SEARCH_BATCH_BYTES", str(20 * (4 * (n + m) + 4 * n + 16 * k)))  # 20 queries a batch: 4 batches
    many = sa.hip_search(db, queries, scoring, k=k, rect=True)
    bd = sa.last_search_breakdown()
    assert bd["batches"] >= 3, bd
    assert sa.last_search_seconds() == pytest.approx(bd["align"] + bd["gather"] + bd["hits"]) and bd["align"] > 0
    for a, b in zip(one, many):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(many[2], want)
    assert_same_hits(many[:2], expected_hits(want, k), "batched")


# ---- 5. hits on synthetic rectangles ---------------------------------------------------------------------------------------
def synthetic(kind: str, m: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * m + n)
    if kind == "three":
        return rng.choice(np.array([-7, 0, 12], np.int32), size=(m, n))
    if kind == "equal":
        return np.full((m, n), 5, np.int32)
    return rng.integers(-2 ** 31, 2 ** 31, size=(m, n), dtype=np.int64).astype(np.int32)


@pytest.fixture(scope="module")
def tiny_contexts(sa):
    """search contexts of N + M one-residue sequences: sa_ctx_hits reads N and the bound on nq from its context only"""
    made = {}

    def get(m, n):
        if (m, n) not in made:
            scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
            made[(m, n)] = sa.SearchContext(sa.SequenceStore.from_sequences([b"A"] * n), sa.SequenceStore.from_sequences([b"A"] * m), scoring, 0)
        return made[(m, n)]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("kind,m,n", [("three", 2, 200_000), ("three", 3, 65), ("random", 3000, 70), ("random", 5, 1), ("equal", 4, 130)])
def test_hits_of_synthetic_rectangles(kind, m, n, sa, tiny_contexts):
    import torch
    rect = synthetic(kind, m, n)
    ctx = tiny_contexts(m, n)
    d_rect = torch.from_numpy(rect).cuda()
    tail = 4096
    stream = torch.cuda.Stream()
    split = []
    for k in sorted({1, min(7, n), min(n, 64)}):
        need = sa.hits_scratch_bytes(n, m, k)
        split.append(need > 0)
        d_index = torch.full((m * k + tail,), POISON, dtype=torch.int32, device="cuda")
        d_score = torch.full((m * k + tail,), POISON, dtype=torch.int32, device="cuda")
        d_scratch = torch.full((need // 4 + tail,), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.hits(d_rect.data_ptr(), m, k, d_index.data_ptr(), d_score.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        index, score, scratch = d_index.cpu().numpy(), d_score.cpu().numpy(), d_scratch.cpu().numpy()
        assert (index[m * k:] == POISON).all() and (score[m * k:] == POISON).all() and (scratch[need // 4:] == POISON).all(), "written beyond the outputs"
        got = index[:m * k].reshape(m, k), score[:m * k].reshape(m, k)
        assert_same_hits(got, expected_hits(rect, k), f"{kind} ({m}, {n}) k={k}")
        if kind == "equal":
            assert (got[0] == np.arange(k)).all()
    assert np.array_equal(d_rect.cpu().numpy(), rect)  # (the input is read only)
    # the paths the shapes are here for
    assert any(split) == ((m, n) in ((2, 200_000), (3, 65), (4, 130))), split
    for bad_k in (0, n + 1, 65):
        with pytest.raises(sa.AlignError, match="k must be in"):
            ctx.hits(d_rect.data_ptr(), m, bad_k, d_rect.data_ptr(), d_rect.data_ptr(), 0)
    with pytest.raises(sa.AlignError, match="queries"):
        ctx.hits(d_rect.data_ptr(), m + 1, 1, d_rect.data_ptr(), d_rect.data_ptr(), 0)


# ---- 6. hits end to end, with ties ------------------------------------------------------------------------------------------
_dna = {}


def dna_case(sa, oracle):
    if not _dna:
        seqs = make_dna_set(300, 120, 180, 4)
        scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
        _dna["case"] = (seqs[:260], seqs[260:], scoring, oracle_rect(sa, oracle, seqs[:260], seqs[260:], scoring))
    return _dna["case"]


@pytest.mark.parametrize("k", [8, 32, 64])
def test_hits_with_ties_across_the_cut(k, sa, oracle):
    db_seqs, query_seqs, scoring, want = dna_case(sa, oracle)
    best = -np.sort(-want.astype(np.int64), axis=1)
    tied = int(np.count_nonzero(best[:, k - 1] == best[:, k]))
    print(f"k = {k}: {tied} of {len(query_seqs)} query rows have equal k-th and (k+1)-th best scores")
    assert tied >= len(query_seqs) // 10  # from the oracle alone, before the device is asked
    index, score, rect = sa.hip_search(sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring, k=k, rect=True)
    assert np.array_equal(rect, want)
    assert_same_hits((index, score), expected_hits(want, k), f"ties k={k}")


# ---- 7. alignments of hits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_alignments_of_hits(method, sa, oracle):
    n, m, k = 700, 65, 3
    db, queries, scoring, want, db_seqs, query_seqs = protein_case(sa, oracle, method, n, m)
    index, score = expected_hits(want, k)
    pairs = [(n + q, int(index[q, t])) for q in range(m) for t in range(k)]
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        got = ctx.alignments(pairs)
    ref = sa.hip_alignments(sa.SequenceStore.from_sequences(list(db_seqs) + list(query_seqs)), scoring, pairs)
    assert np.array_equal(got.records["score"], score.reshape(-1)), "a record's score is not the hit's"
    assert got.records.tobytes() == ref.records.tobytes(), "spans differ from hip_alignments on the concatenated store"
    assert np.array_equal(got.cigar, ref.cigar)
