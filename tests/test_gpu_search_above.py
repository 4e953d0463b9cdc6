"""GPU (-m gpu): every hit of a search at or above a threshold, as a CSR over the rows of the rectangle
(sa_ctx_hits_above_offsets / sa_ctx_hits_above_fill / sa_hip_search_above, csrc/sa_search_above.hip).  Contract
(include/seqalign_hip.h): database sequence d is a hit of row r iff vrect[r, d] >= min_value; offsets int64[nq + 1]; index in
ascending d per row; value = vrect and score = rect at each hit; any int32 threshold; the same inputs give the same bytes.

The expectation never comes from the code under test: it is np.nonzero(vrect >= t), row by row, on a synthetic rectangle or on a
rectangle built from the oracle's scores -- the value rectangles by NumPy int64 floor division (tests/test_gpu_normalize.py:
normalized) and, for percent identity, by the triangle form of the identity sweep on the concatenated store, which
tests/test_gpu_identity.py pins to the plain-Python restatement; whole rows of it are compared here with that restatement
(tests/traceback_ref.py, python_pid) before the device is asked -- all 45 500 pairs in plain Python would take most of a minute.
Everything is compared exactly.

1. synthetic rectangles: five shapes (one step and a tail, a cut off 64, thousands of segments, rows that fill the device), three
   kinds of content, four thresholds, four ways to call; poisoned tails, inputs unchanged, the split asserted
2. refusals that need a context
3. one rectangle past 2^31 elements
4. end to end against the oracle: raw scores, a normalised kind, an identity kind; batches; alignments of the hits"""
import numpy as np
import pytest

from tests.search_cases import oracle_rect
from tests.synth import make_protein_set
from tests.test_gpu_identity import SHORTER, python_pid, reference
from tests.test_gpu_normalize import MIN, SELF, normalized

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
POISON = -0x5A5A5A5B
POISON64 = -0x5A5A5A5A5A5A5A5B
TAIL = 4096


def expected_csr(vrect: np.ndarray, rect: np.ndarray, t: int):
    """offsets, index, value, score of the contract: np.nonzero per row, rows in order"""
    m = vrect.shape[0]
    offsets = np.zeros(m + 1, np.int64)
    index, value, score = [], [], []
    for q in range(m):
        d = np.nonzero(vrect[q] >= t)[0]
        offsets[q + 1] = offsets[q] + len(d)
        index.append(d.astype(np.int32))
        value.append(vrect[q, d])
        score.append(rect[q, d])
    return offsets, np.concatenate(index), np.concatenate(value).astype(np.int32), np.concatenate(score).astype(np.int32)


def assert_same_csr(got, want, what):
    for name, g, w in zip(("offsets", "index", "value", "score"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} of {w.size} entries of {name} differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"


# ---- 1. synthetic rectangles -----------------------------------------------------------------------------------------------------
def synthetic(kind: str, m: int, n: int, seed: int = 0) -> np.ndarray:
    """the kinds of tests/test_gpu_search.py: three distinct values, all equal, the whole int32 range"""
    rng = np.random.default_rng(1000 * m + n + seed)
    if kind == "three":
        return rng.choice(np.array([-7, 0, 12], np.int32), size=(m, n))
    if kind == "equal":
        return np.full((m, n), 5, np.int32)
    return rng.integers(-2 ** 31, 2 ** 31, size=(m, n), dtype=np.int64).astype(np.int32)


@pytest.fixture(scope="module")
def above_contexts(sa):
    """search contexts of N + M one-residue sequences: the calls read N and the bound on nq from their context only"""
    made = {}

    def get(m, n):
        if (m, n) not in made:
            scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
            made[(m, n)] = sa.SearchContext(sa.SequenceStore.from_sequences([b"A"] * n), sa.SequenceStore.from_sequences([b"A"] * m), scoring, 0)
        return made[(m, n)]
    yield get
    for ctx in made.values():
        ctx.close()


# segments per row (include/seqalign_hip.h: sa_hits_above_scratch_bytes = 8 * (nq * S + 1)): one step and a one-lane tail; a cut at 65;
# N / 64 segments with bounds off 64; rows that fill the device by themselves
SHAPES = {(5, 1): 1, (3, 65): 1, (4, 130): 2, (2, 200_003): 3125, (3000, 70): 1}
MIDDLE = {"three": 0, "equal": 5, "random": 0}


def run_above(sa, ctx, d_vrect, d_rect, m, n, t, e, want_value=True, want_score=True, stream=None):
    """offsets, then fill, into poisoned buffers of exactly the contract's sizes + TAIL; returns host arrays (None: not asked for)"""
    import torch
    need = sa.hits_above_scratch_bytes(n, m)
    assert need % 8 == 0
    d_offsets = torch.full((m + 1 + TAIL,), POISON64, dtype=torch.int64, device="cuda")
    d_scratch = torch.full((need // 8 + TAIL,), POISON64, dtype=torch.int64, device="cuda")
    out = [torch.full((e + TAIL,), POISON, dtype=torch.int32, device="cuda") if want else None for want in (True, want_value, want_score)]
    torch.cuda.synchronize()
    s = stream.cuda_stream if stream is not None else 0
    ctx.hits_above_offsets(d_vrect.data_ptr(), m, t, d_offsets.data_ptr(), d_scratch.data_ptr(), stream=s)
    (stream if stream is not None else torch.cuda).synchronize()
    offsets = d_offsets.cpu().numpy()
    assert (offsets[m + 1:] == POISON64).all(), "offsets: written beyond nq + 1"
    assert offsets[m] == e, f"E = {offsets[m]}, want {e}"  # (the fill's buffers are sized by the expectation)
    ctx.hits_above_fill(d_vrect.data_ptr(), d_rect.data_ptr() if d_rect is not None else 0, m, t, d_offsets.data_ptr(), d_scratch.data_ptr(),
                        *(o.data_ptr() if o is not None else 0 for o in out), stream=s)
    (stream if stream is not None else torch.cuda).synchronize()
    scratch = d_scratch.cpu().numpy()
    assert (scratch[need // 8:] == POISON64).all(), "scratch: written beyond its size"
    assert scratch[need // 8 - 1] == e, "the total behind the scanned counts"
    assert (d_offsets.cpu().numpy() == offsets).all(), "the fill changed the offsets"
    host = []
    for name, o in zip(("index", "value", "score"), out):
        if o is None:
            host.append(None)
            continue
        a = o.cpu().numpy()
        assert (a[e:] == POISON).all(), f"{name}: written beyond E"
        host.append(a[:e])
    return (offsets[:m + 1], *host)


@pytest.mark.parametrize("kind", ["three", "equal", "random"])
@pytest.mark.parametrize("m,n", list(SHAPES))
def test_csr_of_synthetic_rectangles(m, n, kind, sa, above_contexts):
    import torch
    vrect, rect = synthetic(kind, m, n), synthetic("random", m, n, seed=7)
    ctx = above_contexts(m, n)
    assert (ctx.n_db, ctx.n_queries) == (n, m)
    assert sa.hits_above_scratch_bytes(n, m) == 8 * (m * SHAPES[(m, n)] + 1), "the shape does not split as it is here to"
    d_vrect, d_rect = torch.from_numpy(vrect).cuda(), torch.from_numpy(rect).cuda()
    side = torch.cuda.Stream()
    top = int(vrect.max())
    for t in (INT32_MIN, INT32_MAX, min(top + 1, INT32_MAX), MIDDLE[kind]):
        what = f"{kind} ({m}, {n}) t={t}"
        want = expected_csr(vrect, rect, t)
        same = want[:3] + (want[2],)
        e = int(want[0][m])
        if t == INT32_MIN:
            assert e == m * n
        if t > top:
            assert e == 0
        if t == MIDDLE[kind] and m * n >= 64:
            assert 0 < e and (kind == "equal" or e < m * n), "the middle threshold keeps a part"
        assert_same_csr(run_above(sa, ctx, d_vrect, d_rect, m, n, t, e), want, what + ", another rectangle")
        assert_same_csr(run_above(sa, ctx, d_vrect, d_vrect, m, n, t, e), same, what + ", d_rect == d_vrect")
        got = run_above(sa, ctx, d_vrect, None, m, n, t, e, want_value=False, want_score=False)
        assert got[2] is None and got[3] is None
        assert_same_csr(got, want, what + ", index alone")
        assert_same_csr(run_above(sa, ctx, d_vrect, d_rect, m, n, t, e, want_value=False), want, what + ", score without value")
        assert_same_csr(run_above(sa, ctx, d_vrect, d_rect, m, n, t, e, stream=side), want, what + ", side stream")
    assert np.array_equal(d_vrect.cpu().numpy(), vrect) and np.array_equal(d_rect.cpu().numpy(), rect), "an input was written"


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_device_resident_calls(sa, above_contexts):
    """every refusal with its message, nothing launched (the poison stays), each followed by a valid call"""
    import torch
    m, n = 4, 130
    ctx = above_contexts(m, n)
    vrect = synthetic("three", m, n)
    want = expected_csr(vrect, vrect, 0)
    e = int(want[0][m])
    d_vrect = torch.from_numpy(vrect).cuda()
    need = sa.hits_above_scratch_bytes(n, m)
    assert sa.hits_above_scratch_bytes(0, m) == 0 and sa.hits_above_scratch_bytes(n, 0) == 0 and sa.hits_above_scratch_bytes(-3, -3) == 0
    d_off = torch.full((m + 1,), POISON64, dtype=torch.int64, device="cuda")
    d_scr = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device="cuda")
    d_out = torch.full((3 * (e + 1),), POISON, dtype=torch.int32, device="cuda")
    v, o, s, x = d_vrect.data_ptr(), d_off.data_ptr(), d_scr.data_ptr(), d_out.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return (d_off.cpu().numpy() == POISON64).all() and (d_scr.cpu().numpy() == POISON64).all() and (d_out.cpu().numpy() == POISON).all()

    def valid():
        ctx.hits_above_offsets(v, m, 0, o, s)
        ctx.hits_above_fill(v, v, m, 0, o, s, x, x + 4 * (e + 1), x + 8 * (e + 1))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert_same_csr((d_off.cpu().numpy(), out[:e], out[e + 1:2 * e + 1], out[2 * e + 2:3 * e + 2]), want[:3] + (want[2],), "valid call")
        for b, p in ((d_off, POISON64), (d_scr, POISON64), (d_out, POISON)):
            b.fill_(p)
        torch.cuda.synchronize()

    off, fill = "sa_ctx_hits_above_offsets: ", "sa_ctx_hits_above_fill: "
    refusals = [
        (off + "null argument", lambda: ctx.hits_above_offsets(0, m, 0, o, s)),
        (off + "null argument", lambda: ctx.hits_above_offsets(v, m, 0, 0, s)),
        (off + "null argument", lambda: ctx.hits_above_offsets(v, m, 0, o, 0)),
        (off + "0 rows, the context has 4 queries", lambda: ctx.hits_above_offsets(v, 0, 0, o, s)),
        (off + "5 rows, the context has 4 queries", lambda: ctx.hits_above_offsets(v, m + 1, 0, o, s)),
        (off + "-1 rows, the context has 4 queries", lambda: ctx.hits_above_offsets(v, -1, 0, o, s)),
        (off + "scratch not 8-byte aligned", lambda: ctx.hits_above_offsets(v, m, 0, o, s + 4)),
        (fill + "null argument", lambda: ctx.hits_above_fill(0, v, m, 0, o, s, x, x, x)),
        (fill + "null argument", lambda: ctx.hits_above_fill(v, v, m, 0, 0, s, x, x, x)),
        (fill + "null argument", lambda: ctx.hits_above_fill(v, v, m, 0, o, 0, x, x, x)),
        (fill + "null argument", lambda: ctx.hits_above_fill(v, v, m, 0, o, s, 0, x, x)),
        (fill + "null argument", lambda: ctx.hits_above_fill(v, 0, m, 0, o, s, x, x, x)),  # (a score wants its rectangle)
        (fill + "0 rows, the context has 4 queries", lambda: ctx.hits_above_fill(v, v, 0, 0, o, s, x, x, x)),
        (fill + "5 rows, the context has 4 queries", lambda: ctx.hits_above_fill(v, v, m + 1, 0, o, s, x, x, x)),
        (fill + "scratch not 8-byte aligned", lambda: ctx.hits_above_fill(v, v, m, 0, o, s + 4, x, x, x)),
    ]
    for message, call in refusals:
        with pytest.raises(sa.AlignError, match=message):
            call()
        assert untouched(), f"{message}: something was launched"
        valid()
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    with sa.Context(sa.SequenceStore.from_sequences([b"A"] * 8), scoring, 0) as plain:
        for call in (lambda: sa.SearchContext.hits_above_offsets(plain, v, 1, 0, o, s), lambda: sa.SearchContext.hits_above_fill(plain, v, v, 1, 0, o, s, x)):
            with pytest.raises(sa.AlignError, match="not a search context"):
                call()
    assert untouched()
    valid()


# ---- 3. past 2^31 elements -----------------------------------------------------------------------------------------------------------
BIG_N, BIG_M = 66_000, 32_600  # (the shape of tests/test_gpu_search_quantity.py::test_sweep_past_two_to_the_31_elements)
BIG_T = 2**31 - 2**32 // 1000  # the values are spread evenly over all of int32, row by row: the top thousandth


def big_value(r, d):
    """closed form of the synthetic rectangle, torch int64 in, int64 out: the element's number times the golden-ratio multiplier
    modulo 2^32, as a signed 32-bit value -- equidistributed along every row, so every row has its share of the hits (the product
    stays below 2^63)"""
    return ((r * BIG_N + d) * 2_654_435_761) % 2**32 - 2**31


def test_csr_past_two_to_the_31_elements(sa):
    import torch
    elems = BIG_N * BIG_M
    assert elems > 2**31 and elems == 2_151_600_000
    peak = 4 * elems + 16 * 2**30
    if not sa.hip_memory(peak):
        pytest.skip(f"the device has no room for {peak / 2**30:.0f} GiB (and a third more): the rectangle and the workspace of the reference")
    distinct = [make_protein_set(1, 1 + k % 3, 1 + k % 3, 8100 + k)[0] for k in range(12)]
    order = np.random.default_rng(73).integers(0, 12, BIG_N + BIG_M)
    seqs = [distinct[k] for k in order]
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    block = 1024
    cols = torch.arange(BIG_N, dtype=torch.int64, device="cuda")[None, :]
    buf = torch.empty(elems, dtype=torch.int32, device="cuda")
    for r0 in range(0, BIG_M, block):
        r1 = min(r0 + block, BIG_M)
        rows = torch.arange(r0, r1, dtype=torch.int64, device="cuda")[:, None]
        buf[r0 * BIG_N:r1 * BIG_N] = big_value(rows, cols).to(torch.int32).reshape(-1)
    need = sa.hits_above_scratch_bytes(BIG_N, BIG_M)
    assert need == 8 * (BIG_M + 1)  # the rows fill the device by themselves: one segment each
    d_offsets = torch.full((BIG_M + 1 + TAIL,), POISON64, dtype=torch.int64, device="cuda")
    d_scratch = torch.full((need // 8 + TAIL,), POISON64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with sa.SearchContext(sa.SequenceStore.from_sequences(seqs[:BIG_N]), sa.SequenceStore.from_sequences(seqs[BIG_N:]), scoring, 0) as ctx:
        assert (ctx.n_db, ctx.n_queries) == (BIG_N, BIG_M)
        ctx.hits_above_offsets(buf.data_ptr(), BIG_M, BIG_T, d_offsets.data_ptr(), d_scratch.data_ptr())
        torch.cuda.synchronize()
        e = int(d_offsets[BIG_M].item())
        print(f"{e} hits of {elems} candidates ({1e2 * e / elems:.4f} %)")
        assert elems // 2000 < e < elems // 500, "the threshold keeps about a thousandth"  # (from the closed form: sized below by it)
        d_index = torch.full((e + TAIL,), POISON, dtype=torch.int32, device="cuda")
        d_value = torch.full((e + TAIL,), POISON, dtype=torch.int32, device="cuda")
        d_score = torch.full((e + TAIL,), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.hits_above_fill(buf.data_ptr(), buf.data_ptr(), BIG_M, BIG_T, d_offsets.data_ptr(), d_scratch.data_ptr(), d_index.data_ptr(),
                            d_value.data_ptr(), d_score.data_ptr())
        torch.cuda.synchronize()
    assert (d_offsets[BIG_M + 1:] == POISON64).all() and (d_scratch[need // 8:] == POISON64).all()
    assert (d_index[e:] == POISON).all() and (d_value[e:] == POISON).all() and (d_score[e:] == POISON).all(), "written beyond E"
    offsets = d_offsets[:BIG_M + 1]
    at, wrong = 0, []
    for r0 in range(0, BIG_M, block):
        r1 = min(r0 + block, BIG_M)
        rows = torch.arange(r0, r1, dtype=torch.int64, device="cuda")[:, None]
        want = big_value(rows, cols)
        hit = torch.nonzero(want >= BIG_T)  # (row-major: ascending d within a row)
        counts = torch.bincount(hit[:, 0], minlength=r1 - r0)
        want_off = at + torch.cumsum(counts, 0)
        if not torch.equal(offsets[r0 + 1:r1 + 1], want_off):
            wrong.append(f"offsets of queries [{r0}, {r1})")
            break
        k = hit.shape[0]
        vals = want[hit[:, 0], hit[:, 1]].to(torch.int32)
        for name, got, w in (("index", d_index, hit[:, 1].to(torch.int32)), ("value", d_value, vals), ("score", d_score, vals)):
            if not torch.equal(got[at:at + k], w):
                bad = int((got[at:at + k] != w).nonzero()[0])
                wrong.append(f"{name} of queries [{r0}, {r1}): hit {at + bad}: got {int(got[at + bad])}, want {int(w[bad])}")
        at += k
    assert not wrong, "; ".join(wrong[:3])
    assert at == e and int(offsets[0]) == 0
    # offsets cross 2^31 elements of input: hits on both sides, the last one at or above element 2^31
    row_31 = 2**31 // BIG_N
    assert 0 < int(offsets[row_31]) < e and int(offsets[BIG_M]) > int(offsets[row_31 + 1])
    last_row = int((offsets[1:] > offsets[:-1]).nonzero()[-1])
    assert last_row * BIG_N + int(d_index[e - 1]) >= 2**31


# ---- 4. end to end against the oracle ------------------------------------------------------------------------------------------------
E2E_N, E2E_M = 700, 65
_e2e = {}


def e2e_case(sa, oracle):
    """700 database proteins x 65 queries under SW: the oracle's rectangle and the three expected value rectangles (computed once)"""
    if not _e2e:
        db_seqs, query_seqs = make_protein_set(E2E_N, 20, 60, 11), make_protein_set(E2E_M, 20, 60, 12)
        n, m = E2E_N, E2E_M
        scoring = sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1)
        rect = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
        cat = list(db_seqs) + list(query_seqs)
        den = np.array([oracle.pair(scoring, s, s) for s in cat], np.int32)
        norm = normalized(rect, den[None, :n], den[n:, None], MIN)
        # percent identity: the triangle form on the concatenated store, gathered at tri(N + q) + d ...
        at = np.array([[(n + q) * (n + q - 1) // 2 + d for d in range(n)] for q in range(m)], np.int64)
        pid = np.ascontiguousarray(sa.hip_identity(sa.SequenceStore.from_sequences(cat), scoring, denom=SHORTER, identities=False, columns=False)[2][at])
        # ... three whole rows of it against the plain-Python restatement
        lens = [len(s) for s in cat]
        for q in (0, 31, m - 1):
            pairs = [(d, n + q) for d in range(n)]
            score, ident, cols, _ = reference(scoring, cat, pairs)
            assert np.array_equal(score, rect[q]), "the restatement's scores are the oracle's"
            want = np.array([python_pid(int(i), int(c), lens[d], lens[n + q], SHORTER) for i, c, (d, _) in zip(ident, cols, pairs)], np.int64)
            assert np.array_equal(pid[q], want.astype(np.int32)), f"query {q}: the identity rectangle is not the restatement's"
        for a in (rect, norm, pid):
            a.setflags(write=False)
        _e2e["case"] = (sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring, rect, den,
                        {"raw": rect, "norm": norm, "pid": pid})
    return _e2e["case"]


def quantity_of(sa, kind):
    return {"raw": {}, "norm": dict(norm=sa.Norm(SELF, MIN)), "pid": dict(pid=SHORTER)}[kind]


@pytest.mark.parametrize("kind", ["raw", "norm", "pid"])
def test_search_above_equals_the_oracle(kind, sa, oracle, monkeypatch):
    db, queries, scoring, rect, den, values = e2e_case(sa, oracle)
    n, m = E2E_N, E2E_M
    vrect = values[kind]
    cut = int(np.quantile(vrect, 0.99))
    for t in (cut, INT32_MIN, INT32_MAX):
        want = expected_csr(vrect, rect, t)
        e = int(want[0][m])
        if t == cut:
            assert m * n // 200 <= e <= m * n // 20, "the quantile keeps about a hundredth"
        got = sa.hip_search_above(db, queries, scoring, t, **quantity_of(sa, kind))
        assert sa.last_search_breakdown()["batches"] == 1
        assert_same_csr((got.offsets, got.index, got.value, got.score), want, f"{kind} t={t}")
        assert len(got) == e == (m * n if t == INT32_MIN else 0 if t == INT32_MAX else e)
        if kind == "norm":
            assert np.array_equal(got.denominators, den), "the N + M denominators"
        else:
            assert got.denominators is None
        bd = sa.last_search_breakdown()
        assert sa.last_search_above_seconds() > 0 and bd["hits"] == pytest.approx(sa.last_search_above_seconds())
        assert (sa.last_search_quantity_seconds() > 0) == (kind != "raw")
        # batches of about 20 queries (include/seqalign_hip.h: sa_hip_search_above): the same bytes
        per_query = (4 * (n + m) if kind != "pid" else 0) + (4 if kind == "raw" else 8) * n + 8
        monkeypatch.setenv("SA_HIP_SEARCH_BATCH_BYTES", str(20 * per_query))
        many = sa.hip_search_above(db, queries, scoring, t, **quantity_of(sa, kind))
        monkeypatch.delenv("SA_HIP_SEARCH_BATCH_BYTES")
        assert sa.last_search_breakdown()["batches"] >= 3, sa.last_search_breakdown()
        for name in ("offsets", "index", "value", "score"):
            assert getattr(many, name).tobytes() == getattr(got, name).tobytes(), f"{kind} t={t}: {name} differs between one batch and several"


def test_both_quantities_are_refused_and_the_process_lives_on(sa, oracle):
    db, queries, scoring, rect, _, values = e2e_case(sa, oracle)
    with pytest.raises(sa.AlignError, match="sa_hip_search_above: norm and pid_denom exclude each other"):
        sa.hip_search_above(db, queries, scoring, 0, norm=sa.Norm(SELF, MIN), pid=SHORTER)
    with pytest.raises(sa.AlignError, match="sa_hip_search_above: denom 4 is none of"):
        sa.hip_search_above(db, queries, scoring, 0, pid=4)
    t = int(rect.max())
    got = sa.hip_search_above(db, queries, scoring, t)
    assert_same_csr((got.offsets, got.index, got.value, got.score), expected_csr(rect, rect, t), "the maximum itself")
    assert len(got) >= 1


def test_alignments_of_the_hits(sa, oracle):
    db, queries, scoring, rect, _, values = e2e_case(sa, oracle)
    n, m = E2E_N, E2E_M
    got = sa.hip_search_above(db, queries, scoring, int(np.quantile(values["pid"], 0.99)), pid=SHORTER)
    pairs = [(n + q, int(d)) for q in range(m) for d in got.index[got.row(q)]]
    assert len(pairs) == len(got) >= m
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        alns = ctx.alignments(pairs)
    want = np.array([rect[a - n, b] for a, b in pairs], np.int32)
    assert np.array_equal(alns.records["score"], want), "a record's score is not rect[q, d]"
    assert np.array_equal(got.score, want)
