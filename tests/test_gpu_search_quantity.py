"""GPU (-m gpu): the hits of a search ranked by a value -- normalised score or percent identity -- instead of the raw score
(sa_ctx_normalize_rect / sa_ctx_identity_rect / sa_ctx_hits_take / sa_hip_search_norm / sa_hip_search_pid,
csrc/sa_search_quantity.hip; the rectangle form of sa_k_identity in csrc/sa_identity.hip).  Contract (include/seqalign_hip.h):
the pair of query q and database sequence d is (d, N + q) of the concatenated store; values in parts per million; hits by value
descending, then d ascending; every hit carries its raw score.

The expectation never comes from the code under test: the sweep against NumPy / torch int64 floor division, the identity rectangle
against tests/traceback_ref.py (plain Python) and against the triangle form that is already pinned to it, the hits against NumPy's
lexsort of a value rectangle built from the oracle's scores and self-scores.  Everything is compared exactly.

1. the sweep on synthetic rectangles: shapes around the piece, three rules, in and out of place, views off 16-byte alignment
2. the sweep past 2^31 elements
3. the identity rectangle against the Python restatement, five scorings, the tie rule shown to matter
4. the identity rectangle beyond the resident waves, against the triangle form
5. hits by value with ties across the cut, six normalised and four identity kinds
6. batches"""
import numpy as np
import pytest

from tests import tables
from tests.search_cases import expected_hits, oracle_rect
from tests.synth import make_dna_set, make_protein_set
from tests.test_gpu_identity import COLUMNS, DENOMS, python_pid, reference
from tests.test_gpu_normalize import INT32_MAX, INT32_MIN, LENGTH, MAX, MEAN, MIN, SCALE, SELF, normalized
from tests.test_gpu_search import tiny_contexts  # noqa: F401  (a fixture)
from tests.test_gpu_traceback import CONTRACT_SCORINGS, tie_heavy_sequences
from tests.test_gpu_wave_trips import resident_waves

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B
RULES = (MIN, MAX, MEAN)


# ---- 1. the sweep on synthetic rectangles ------------------------------------------------------------------------------------------
def denominators_for(n, m, seed):
    """as tests/test_gpu_normalize.py has them: all SCALE, all 1, a mix with 0, -5, 1, 7, SCALE, INT32_MAX, INT32_MIN"""
    rng = np.random.default_rng(seed)
    special = np.array([0, -5, 1, 7, SCALE, INT32_MAX, INT32_MIN], np.int32)
    mixed = rng.integers(1, 2001, n + m).astype(np.int32)
    mixed[rng.permutation(n + m)[:min(n + m, 7)]] = rng.permutation(special)[:min(n + m, 7)]
    return {"scale": np.full(n + m, SCALE, np.int32), "ones": np.ones(n + m, np.int32), "mix": mixed}


def expected_values(rect, den, n, q0, rule):
    """rows of `rect` are queries q0 ..: value of (r, d) under den[d] and den[n + q0 + r]"""
    nq = rect.shape[0]
    return normalized(rect, den[None, :n], den[n + q0:n + q0 + nq, None], rule)


@pytest.mark.parametrize("q0", [0, 2])
@pytest.mark.parametrize("n,nq", [(1, 1), (3, 5), (63, 2), (65, 3), (1027, 4)])
def test_sweep_equals_numpy_floor_division(n, nq, q0, sa, tiny_contexts):  # noqa: F811
    import torch
    m = nq + 3
    rng = np.random.default_rng(1000 * n + 10 * nq + q0)
    rect = rng.integers(INT32_MIN, INT32_MAX, (nq, n), endpoint=True).astype(np.int32)
    flat = rect.reshape(-1)
    flat[0] = INT32_MIN
    flat[-1] = INT32_MAX if flat.size > 1 else INT32_MIN
    small = rng.integers(-50000, 50000, (nq, n)).astype(np.int32)  # (ratios that do not saturate: the floor rule shows)
    ctx = tiny_contexts(m, n)
    assert (ctx.n_db, ctx.n_queries) == (n, m)
    stream = torch.cuda.Stream()
    rows_before, rows_after, tail = 2, 2, 64
    negative_inexact = 0
    for name, den in denominators_for(n, m, n + nq).items():
        if name == "mix" and n + m >= 7:
            assert {0, -5, 1, 7, SCALE, INT32_MAX, INT32_MIN} <= set(den.tolist())
        d_den = torch.from_numpy(den).cuda()
        for rule in RULES:
            for scores in (rect, small):
                want = expected_values(scores, den, n, q0, rule)
                if name == "scale":
                    assert np.array_equal(want, scores)  # identity
                dd = {MIN: np.minimum, MAX: np.maximum, MEAN: np.add}[rule](den[None, :n].astype(np.int64), den[n + q0:n + q0 + nq, None].astype(np.int64))
                num = scores.astype(np.int64) * SCALE * (2 if rule == MEAN else 1)
                negative_inexact += int(((dd > 0) & (num < 0) & (num % np.where(dd > 0, dd, 1) != 0) & (want > INT32_MIN)).sum())
                # the rows sit between poisoned rows; out of place on a stream of its own, then in place
                room = (rows_before + nq + rows_after) * n + tail
                src = torch.full((room,), POISON, dtype=torch.int32, device="cuda")
                dst = torch.full((room,), POISON, dtype=torch.int32, device="cuda")
                lo, hi = rows_before * n, (rows_before + nq) * n
                src[lo:hi] = torch.from_numpy(scores.reshape(-1)).cuda()
                torch.cuda.synchronize()
                ctx.normalize_rect(src.data_ptr() + 4 * lo, nq, q0, d_den.data_ptr(), rule, dst.data_ptr() + 4 * lo, stream=stream.cuda_stream)
                stream.synchronize()
                got, kept = dst.cpu().numpy(), src.cpu().numpy()
                bad = np.argwhere(got[lo:hi].reshape(nq, n) != want)
                assert bad.size == 0, (f"({n}, {nq}) q0 {q0} {name} rule {rule}: {len(bad)} entries differ, first at row {bad[0][0]} d {bad[0][1]}: "
                                       f"s {scores[tuple(bad[0])]} d {den[bad[0][1]]}, {den[n + q0 + bad[0][0]]}: got "
                                       f"{got[lo:hi].reshape(nq, n)[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
                assert (got[:lo] == POISON).all() and (got[hi:] == POISON).all(), "written outside the rows"
                assert np.array_equal(kept[lo:hi], scores.reshape(-1)) and (kept[:lo] == POISON).all() and (kept[hi:] == POISON).all()
                ctx.normalize_rect(src.data_ptr() + 4 * lo, nq, q0, d_den.data_ptr(), rule, src.data_ptr() + 4 * lo, stream=stream.cuda_stream)
                stream.synchronize()
                got = src.cpu().numpy()
                assert np.array_equal(got[lo:hi].reshape(nq, n), want), f"({n}, {nq}) q0 {q0} {name} rule {rule}: in place"
                assert (got[:lo] == POISON).all() and (got[hi:] == POISON).all(), "in place: written outside the rows"
                assert np.array_equal(d_den.cpu().numpy(), den)
    if n * nq >= 15:
        print(f"({n}, {nq}) q0 {q0}: {negative_inexact} negative quotients that are no exact multiples")
        assert negative_inexact >= 4  # the floor rule is exercised: truncation misses every one of them by one


@pytest.mark.parametrize("shift_in,shift_out", [(1, 1), (1, 0), (3, 2), (2, 3), (0, 1)])
def test_sweep_on_views_off_the_16_byte_alignment(shift_in, shift_out, sa, tiny_contexts):  # noqa: F811
    """views one to three elements off 16-byte alignment, source and destination independently; N = 1027 puts every row at another
    alignment as well (1027 = 3 mod 4)"""
    import torch
    n, nq, q0 = 1027, 4, 2
    m = nq + 3
    rng = np.random.default_rng(77)
    scores = rng.integers(-50000, 50000, (nq, n)).astype(np.int32)
    den = rng.integers(1, 2001, n + m).astype(np.int32)
    want = expected_values(scores, den, n, q0, MEAN)
    assert ((want < 0) & ((2 * scores.astype(np.int64) * SCALE) % (den[None, :n].astype(np.int64) + den[n + q0:n + q0 + nq, None]) != 0)).sum() > scores.size // 4
    ctx = tiny_contexts(m, n)
    p = nq * n
    room = p + 64 + 4
    src = torch.full((room,), POISON, dtype=torch.int32, device="cuda")
    dst = torch.full((room,), POISON, dtype=torch.int32, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    src[shift_in:shift_in + p] = torch.from_numpy(scores.reshape(-1)).cuda()
    d_den = torch.from_numpy(den).cuda()
    torch.cuda.synchronize()
    ctx.normalize_rect(src.data_ptr() + 4 * shift_in, nq, q0, d_den.data_ptr(), MEAN, dst.data_ptr() + 4 * shift_out)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[shift_out:shift_out + p].reshape(nq, n), want)
    assert (got[:shift_out] == POISON).all() and (got[shift_out + p:] == POISON).all()
    ctx.normalize_rect(src.data_ptr() + 4 * shift_in, nq, q0, d_den.data_ptr(), MEAN, src.data_ptr() + 4 * shift_in)
    torch.cuda.synchronize()
    got = src.cpu().numpy()
    assert np.array_equal(got[shift_in:shift_in + p].reshape(nq, n), want)
    assert (got[:shift_in] == POISON).all() and (got[shift_in + p:] == POISON).all()


def test_refusals_of_the_rectangle_calls(sa, tiny_contexts):  # noqa: F811
    """every refusal with its message, nothing launched (the poison stays), each followed by a valid call"""
    import torch
    n, m = 65, 6
    ctx = tiny_contexts(m, n)
    rect = np.arange(m * n, dtype=np.int32).reshape(m, n) - 100
    den = np.arange(1, n + m + 1, dtype=np.int32)
    d_rect, d_den = torch.from_numpy(rect.reshape(-1)).cuda(), torch.from_numpy(den).cuda()
    d_out = torch.full((m * n + 4,), POISON, dtype=torch.int32, device="cuda")
    index = np.stack([np.arange(q, q + 3) for q in range(m)]).astype(np.int32)
    d_index = torch.from_numpy(index.reshape(-1)).cuda()
    r, d, o, x = d_rect.data_ptr(), d_den.data_ptr(), d_out.data_ptr(), d_index.data_ptr()

    def valid():
        ctx.normalize_rect(r, m, 0, d, MIN, o)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[:m * n].reshape(m, n), expected_values(rect, den, n, 0, MIN))
        d_out.fill_(POISON)
        ctx.hits_take(r, m, 3, x, o)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[:m * 3].reshape(m, 3), np.take_along_axis(rect, index, 1))
        d_out.fill_(POISON)
        torch.cuda.synchronize()

    refusals = [
        ("null argument", lambda: ctx.normalize_rect(0, m, 0, d, MIN, o)),
        ("null argument", lambda: ctx.normalize_rect(r, m, 0, 0, MIN, o)),
        ("null argument", lambda: ctx.normalize_rect(r, m, 0, d, MIN, 0)),
        ("rule 3 is none of", lambda: ctx.normalize_rect(r, m, 0, d, 3, o)),
        ("rule -1 is none of", lambda: ctx.normalize_rect(r, m, 0, d, -1, o)),
        (r"queries \[-1,\+1\) of 6", lambda: ctx.normalize_rect(r, 1, -1, d, MIN, o)),
        (r"queries \[0,\+0\) of 6", lambda: ctx.normalize_rect(r, 0, 0, d, MIN, o)),
        (r"queries \[2,\+5\) of 6", lambda: ctx.normalize_rect(r, 5, 2, d, MIN, o)),
        (r"queries \[6,\+1\) of 6", lambda: ctx.normalize_rect(r, 1, 6, d, MIN, o)),
        ("4-byte alignment", lambda: ctx.normalize_rect(r + 2, m, 0, d, MIN, o)),
        ("4-byte alignment", lambda: ctx.normalize_rect(r, m, 0, d + 1, MIN, o)),
        ("4-byte alignment", lambda: ctx.normalize_rect(r, m, 0, d, MIN, o + 3)),
        ("sa_ctx_identity_rect: every output is null", lambda: ctx.identity_rect(0, m)),
        ("sa_ctx_identity_rect: denom 4 is none of", lambda: ctx.identity_rect(0, m, pid=o, denom=4)),
        (r"sa_ctx_identity_rect: queries \[5,\+2\) of 6", lambda: ctx.identity_rect(5, 2, score=o)),
        (r"sa_ctx_identity_rect: queries \[0,\+0\) of 6", lambda: ctx.identity_rect(0, 0, score=o)),
        ("sa_ctx_identity_rect: the outputs want 4-byte alignment", lambda: ctx.identity_rect(0, 1, columns=o + 2)),
        ("sa_ctx_hits_take: null argument", lambda: ctx.hits_take(r, m, 3, 0, o)),
        ("sa_ctx_hits_take: null argument", lambda: ctx.hits_take(0, m, 3, x, o)),
        ("sa_ctx_hits_take: k = 0 hits", lambda: ctx.hits_take(r, m, 0, x, o)),
        ("sa_ctx_hits_take: k = 66 hits", lambda: ctx.hits_take(r, m, 66, x, o)),
        ("sa_ctx_hits_take: 7 rows, the context has 6 queries", lambda: ctx.hits_take(r, m + 1, 3, x, o)),
        ("sa_ctx_hits_take: .* 4-byte alignment", lambda: ctx.hits_take(r, m, 3, x + 2, o)),
    ]
    for message, call in refusals:
        with pytest.raises(sa.AlignError, match=message):
            call()
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == POISON).all(), f"{message}: something was launched"
        valid()
    # a plain context refuses the three calls; a search context keeps refusing the packed ones (tests/test_gpu_search.py pins that)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    with sa.Context(sa.SequenceStore.from_sequences([b"A"] * 8), scoring, 0) as plain:
        for call in (lambda: sa.SearchContext.normalize_rect(plain, r, 1, 0, d, MIN, o), lambda: sa.SearchContext.identity_rect(plain, 0, 1, score=o),
                     lambda: sa.SearchContext.hits_take(plain, r, 1, 1, x, o)):
            with pytest.raises(sa.AlignError, match="not a search context"):
                call()
    for call in (lambda: ctx.normalize(r, d, MIN, o), lambda: ctx.identity_range(0, 16, score=o)):
        with pytest.raises(sa.AlignError, match="sa_ctx_search_range"):
            call()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == POISON).all()
    valid()


def test_denominators_of_a_search_context_are_those_of_the_concatenated_store(sa, oracle):
    """N + M values, database first: lengths, and self-scores by the full DP (the oracle's pair of a sequence with itself)"""
    import torch
    db_seqs, query_seqs = make_protein_set(70, 1, 90, 31), make_protein_set(9, 1, 90, 32)
    n, m = len(db_seqs), len(query_seqs)
    for method in tables.METHODS:
        scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
        with sa.SearchContext(sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring, 0) as ctx:
            for source, want in ((LENGTH, [len(s) for s in db_seqs + query_seqs]), (SELF, [oracle.pair(scoring, s, s) for s in db_seqs + query_seqs])):
                d = torch.full((n + m + 64,), POISON, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ctx.denominators(source, d.data_ptr())
                torch.cuda.synchronize()
                got = d.cpu().numpy()
                assert got[:n + m].tolist() == want and (got[n + m:] == POISON).all(), f"{method} source {source}"


# ---- 2. past 2^31 elements ----------------------------------------------------------------------------------------------------------
BIG_N, BIG_M = 66_000, 32_600


def big_value(r, d):
    """closed form of the synthetic rectangle, torch int64 in, int64 out: about +-2^29, every residue class of small moduli"""
    return ((r * 1_000_003 + d * 7_919 + (r ^ d) * 31) % (2**30 + 7)) - 2**29


def big_denominators():
    k = np.arange(BIG_N + BIG_M, dtype=np.int64)
    d = 2**20 + (k * 2_654_435_761) % (2**30)
    d = np.where(k % 101 == 5, -d, d)
    return np.where(k % 97 == 3, 0, d).astype(np.int32)


def test_sweep_past_two_to_the_31_elements(sa):
    import time

    import torch
    from tests import synth_triangle as st
    elems = BIG_N * BIG_M
    assert elems > 2**31 and elems == 2_151_600_000
    peak = 4 * elems + 16 * 2**30
    if not sa.hip_memory(peak):
        pytest.skip(f"the device has no room for {peak / 2**30:.0f} GiB (and a third more): the rectangle and the workspace of the reference")
    distinct = [make_protein_set(1, 1 + k % 3, 1 + k % 3, 8100 + k)[0] for k in range(12)]
    order = np.random.default_rng(73).integers(0, 12, BIG_N + BIG_M)
    seqs = [distinct[k] for k in order]
    assert {len(s) for s in seqs} == {1, 2, 3}
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    den = big_denominators()
    d_den = torch.from_numpy(den).cuda()
    den64 = d_den.to(torch.int64)
    block = 1024
    cols = torch.arange(BIG_N, dtype=torch.int64, device="cuda")[None, :]
    buf = torch.empty(elems + 1, dtype=torch.int32, device="cuda")
    buf[elems] = POISON
    for r0 in range(0, BIG_M, block):
        r1 = min(r0 + block, BIG_M)
        rows = torch.arange(r0, r1, dtype=torch.int64, device="cuda")[:, None]
        buf[r0 * BIG_N:r1 * BIG_N] = big_value(rows, cols).to(torch.int32).reshape(-1)
    torch.cuda.synchronize()
    with sa.SearchContext(sa.SequenceStore.from_sequences(seqs[:BIG_N]), sa.SequenceStore.from_sequences(seqs[BIG_N:]), scoring, 0) as ctx:
        assert (ctx.n_db, ctx.n_queries) == (BIG_N, BIG_M)
        t0 = time.perf_counter()
        ctx.normalize_rect(buf.data_ptr(), BIG_M, 0, d_den.data_ptr(), MEAN, buf.data_ptr())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    assert buf[elems].item() == POISON, "written beyond nq * N elements"
    wrong, count, seen = [], 0, set()
    for r0 in range(0, BIG_M, block):
        r1 = min(r0 + block, BIG_M)
        rows = torch.arange(r0, r1, dtype=torch.int64, device="cuda")[:, None]
        want = st.normalized(big_value(rows, cols), den64[None, :BIG_N], den64[BIG_N + r0:BIG_N + r1, None], 2).to(torch.int32)
        got = buf[r0 * BIG_N:r1 * BIG_N].reshape(r1 - r0, BIG_N)
        bad = (got != want).nonzero()
        if bad.numel():
            count += bad.shape[0]
            for at in ([bad[0], bad[-1]] if not wrong else [bad[-1]]):
                r, d = int(at[0]), int(at[1])
                side = "below 2^31" if (r0 + r) * BIG_N + d < 2**31 else "at or above 2^31"
                wrong.append(f"query {r0 + r}, d {d} (element {(r0 + r) * BIG_N + d}, {side}): got {got[r, d].item()}, want {want[r, d].item()}")
        seen |= {int(want.min()), int((want < 0).sum() > 0)}
    torch.cuda.synchronize()
    print(f"sweep over {elems} elements in place: {1e3 * (t1 - t0):.1f} ms ({8 * elems / (t1 - t0) / 1e12:.2f} TB/s at 8 bytes per entry), "
          f"floor division over all row blocks {time.perf_counter() - t1:.2f} s")
    assert not wrong, f"{count} entries differ; first " + wrong[0] + "; last " + wrong[-1]
    assert INT32_MIN in seen and 1 in seen  # a denominator <= 0 and negative quotients are compared too


# ---- 3. the identity rectangle against the restatement ---------------------------------------------------------------------------------
IDENTITY_SCORINGS = [(m, x, g) for m, x, g in CONTRACT_SCORINGS[:3]] + [("nw", "blosum62", dict(gap_pen=0)), ("ga", "asym", tables.GAPS["ga"])]


def device_identity_rect(ctx, q0, nq, n, denom=COLUMNS, want=("score", "identities", "columns", "pid"), stream=0):
    """the outputs asked for, each between a poisoned row before and 64 poisoned elements behind"""
    import torch
    count = nq * n
    bufs = {name: torch.full((n + count + 64,), POISON, dtype=torch.int32, device="cuda") for name in want}
    torch.cuda.synchronize()
    ctx.identity_rect(q0, nq, denom=denom, stream=stream, **{name: b.data_ptr() + 4 * n for name, b in bufs.items()})
    torch.cuda.synchronize()
    got = {}
    for name, b in bufs.items():
        host = b.cpu().numpy()
        assert (host[:n] == POISON).all() and (host[n + count:] == POISON).all(), f"sa_ctx_identity_rect wrote outside the rows in {name}"
        got[name] = host[n:n + count].reshape(nq, n).copy()
    return got


@pytest.mark.parametrize("method,matrix,gaps", IDENTITY_SCORINGS, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_identity_rectangle_equals_the_python_restatement(method, matrix, gaps, sa, oracle):
    import torch
    seqs = make_protein_set(30, 1, 80, 11) + tie_heavy_sequences()
    n = m = len(seqs)
    assert n == 45
    scoring = tables.scoring_with(sa, method, gaps, tables.asym(), lut=sa.Scoring.from_names(method, "blosum62", **gaps).lut) if matrix == "asym" \
        else sa.Scoring.from_names(method, matrix, **gaps)
    cat = seqs + seqs
    lens = [len(s) for s in cat]
    pairs = [(d, n + q) for q in range(m) for d in range(n)]  # self pairs and both orientations of every pair are among them
    assert len(pairs) == 2025 and max(lens) == 80 > 64  # two strips
    score, ident, cols, changed = reference(scoring, cat, pairs, flipped=True)
    score, ident, cols = (a.reshape(m, n) for a in (score, ident, cols))
    store = sa.SequenceStore.from_sequences(seqs)
    assert np.array_equal(score, oracle_rect(sa, oracle, seqs, seqs, scoring))  # the restatement's scores are the oracle's
    empty = int((cols == 0).sum())
    print(f"{method} {matrix} {gaps}: {changed} of 2025 pairs change under the other tie order, {empty} empty alignments")
    if (method, matrix, gaps.get("gap_open"), gaps.get("gap_extend")) != ("sw", "blosum62", 10, 1):
        # (the pairs with d < q are exactly the 990 triangle pairs for which tests/test_gpu_identity.py asserts the same)
        assert changed >= 30, "the case cannot tell the tie rule from another"
    if scoring.method == 2:
        assert empty >= 1  # INT32_MIN under COLUMNS

    def pid_of(denom, q0=0, nq=m):
        return np.array([[python_pid(int(ident[q, d]), int(cols[q, d]), lens[d], lens[n + q], denom) for d in range(n)] for q in range(q0, q0 + nq)],
                        np.int64).astype(np.int32)

    stream = torch.cuda.Stream()
    with sa.SearchContext(store, store, scoring, 0) as ctx:
        for denom in DENOMS:
            got = device_identity_rect(ctx, 0, m, n, denom, stream=stream.cuda_stream if denom == DENOMS[-1] else 0)
            for name, want in (("score", score), ("identities", ident), ("columns", cols), ("pid", pid_of(denom))):
                bad = np.argwhere(got[name] != want)
                assert bad.size == 0, (f"{method} {matrix} {gaps} denom {denom} {name}: {len(bad)} of 2025 differ, first query {bad[0][0]} d {bad[0][1]} "
                                       f"({lens[bad[0][1]]} x {lens[n + bad[0][0]]} residues): got {got[name][tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        if empty:
            assert (device_identity_rect(ctx, 0, m, n, COLUMNS, ("pid",))["pid"] == INT32_MIN).sum() == empty
        # subsets of the outputs, q0 > 0
        for q0, nq, names in ((17, 1, ("pid",)), (42, 3, ("identities", "columns")), (3, 20, ("score", "pid"))):
            got = device_identity_rect(ctx, q0, nq, n, DENOMS[2], names)
            for name, want in (("score", score), ("identities", ident), ("columns", cols)):
                if name in names:
                    assert np.array_equal(got[name], want[q0:q0 + nq]), f"queries [{q0},+{nq}) {name}"
            if "pid" in names:
                assert np.array_equal(got["pid"], pid_of(DENOMS[2], q0, nq)), f"queries [{q0},+{nq}) pid"


# ---- 4. the identity rectangle beyond the resident waves -----------------------------------------------------------------------------
@pytest.mark.parametrize("method", tables.METHODS)
def test_identity_rectangle_on_later_trips_equals_the_triangle_form(method, sa):
    n, m = 260, 70
    w = resident_waves()
    while n * m <= 2 * w:  # (a device with more waves: more queries)
        m += 10
    assert n * m > 2 * w
    distinct = [make_protein_set(1, ln, ln, 500 + ln)[0] for ln in (1, 2, 3, 17, 40, 63, 64, 65, 80, 100, 127, 128, 129, 140)] + make_protein_set(10, 5, 139, 77)
    assert len(set(distinct)) == 24 and {len(s) for s in distinct} >= {1, 64, 65, 128, 129, 140} and max(map(len, distinct)) == 140
    order = np.random.default_rng(91).integers(0, 24, n + m)
    assert len(set(order.tolist())) == 24
    seqs = [distinct[k] for k in order]
    scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
    cat = sa.SequenceStore.from_sequences(seqs)
    ident, cols, pid = sa.hip_identity(cat, scoring, denom=DENOMS[3])  # (pinned to the restatement by tests/test_gpu_identity.py)
    at = np.array([[(n + q) * (n + q - 1) // 2 + d for d in range(n)] for q in range(m)], np.int64)
    with sa.SearchContext(sa.SequenceStore.from_sequences(seqs[:n]), sa.SequenceStore.from_sequences(seqs[n:]), scoring, 0) as ctx:
        got = device_identity_rect(ctx, 0, m, n, DENOMS[3], ("identities", "columns", "pid"))
    for name, want in (("identities", ident[at]), ("columns", cols[at]), ("pid", pid[at])):
        bad = np.argwhere(got[name] != want)
        assert bad.size == 0, (f"{method} {name}: {len(bad)} of {n * m} differ, first query {bad[0][0]} d {bad[0][1]} (wave item {bad[0][0] * n + bad[0][1]}, "
                               f"{w} resident waves): got {got[name][tuple(bad[0])]}, want {want[tuple(bad[0])]}")


# ---- 5. hits by value with ties across the cut -------------------------------------------------------------------------------------------
NORM_KINDS = [(source, rule) for source in (SELF, LENGTH) for rule in RULES]
_tie = {}


def tie_case(sa, oracle):
    """130 distinct DNA sequences each present twice under a fixed shuffle, 40 queries, SW / nuc44 / 10-1; the oracle's rectangle and
    self-scores, the lengths (computed once)"""
    if not _tie:
        distinct = make_dna_set(170, 120, 180, 4)
        db_seqs = [distinct[k] for k in np.random.default_rng(5).permutation(np.repeat(np.arange(130), 2))]
        query_seqs = distinct[130:]
        assert len(db_seqs) == 260 and len(query_seqs) == 40 and len(set(db_seqs)) == 130
        scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
        rect = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
        rect.setflags(write=False)
        den = {SELF: np.array([oracle.pair(scoring, s, s) for s in db_seqs + query_seqs], np.int32),
               LENGTH: np.array([len(s) for s in db_seqs + query_seqs], np.int32)}
        _tie["case"] = (db_seqs, query_seqs, scoring, rect, den)
    return _tie["case"]


def identity_values(sa, db_seqs, query_seqs, scoring):
    """the four pid rectangles by the path of check 4: hip_identity on the concatenated store, gathered at tri(N + q) + d"""
    if "pid" not in _tie:
        n, m = len(db_seqs), len(query_seqs)
        cat = sa.SequenceStore.from_sequences(list(db_seqs) + list(query_seqs))
        at = np.array([[(n + q) * (n + q - 1) // 2 + d for d in range(n)] for q in range(m)], np.int64)
        _tie["pid"] = {denom: np.ascontiguousarray(sa.hip_identity(cat, scoring, denom=denom, identities=False, columns=False)[2][at]) for denom in DENOMS}
    return _tie["pid"]


def check_hits_by_value(sa, what, got, vrect, rect, k):
    index, value, score, got_rect, got_vrect = got[:5]
    m = rect.shape[0]
    assert np.array_equal(got_rect, rect), f"{what}: rect"
    assert np.array_equal(got_vrect, vrect), f"{what}: vrect"
    wi, wv = expected_hits(vrect, k)
    for name, g, w in (("index", index, wi), ("value", value, wv), ("score", score, np.take_along_axis(rect, wi.astype(np.int64), 1))):
        assert g.dtype == np.int32 and g.shape == (m, k), f"{what} k={k} {name}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} k={k} {name}: {len(bad)} entries differ, first at query {bad[0][0]} place {bad[0][1]}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
    return wi


KS = (1, 7, 33, 63, 64)


def assert_ties_across_the_cut(vrect, what):
    best = -np.sort(-vrect.astype(np.int64), axis=1)
    for k in KS[:-1]:  # every value occurs an even number of times: for odd k every row has equal k-th and (k+1)-th values
        tied = int(np.count_nonzero(best[:, k - 1] == best[:, k]))
        assert tied == vrect.shape[0], f"{what} k={k}: {tied} of {vrect.shape[0]} rows tie across the cut"


@pytest.mark.parametrize("source,rule", NORM_KINDS)
def test_hits_by_normalised_score(source, rule, sa, oracle):
    db_seqs, query_seqs, scoring, rect, den = tie_case(sa, oracle)
    n, m = len(db_seqs), len(query_seqs)
    vrect = normalized(rect, den[source][None, :n], den[source][n:, None], rule)
    assert_ties_across_the_cut(vrect, f"source {source} rule {rule}")
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    differs = 0
    for k in KS:
        got = sa.hip_search(db, queries, scoring, k=k, rect=True, norm=sa.Norm(source, rule))
        assert len(got) == 6 and np.array_equal(got[5], den[source]), "the N + M denominators"
        wi = check_hits_by_value(sa, f"source {source} rule {rule}", got, vrect, rect, k)
        differs += int((wi != expected_hits(rect, k)[0]).any(axis=1).sum())
    assert differs >= 1, "ranked by the value the hits are the hits by raw score: the case shows nothing"
    assert sa.last_search_quantity_seconds() > 0


@pytest.mark.parametrize("denom", DENOMS)
def test_hits_by_percent_identity(denom, sa, oracle):
    db_seqs, query_seqs, scoring, rect, _ = tie_case(sa, oracle)
    vrect = identity_values(sa, db_seqs, query_seqs, scoring)[denom]
    assert_ties_across_the_cut(vrect, f"denom {denom}")
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    differs = 0
    for k in KS:
        got = sa.hip_search(db, queries, scoring, k=k, rect=True, pid=denom)
        assert len(got) == 5
        wi = check_hits_by_value(sa, f"denom {denom}", got, vrect, rect, k)
        differs += int((wi != expected_hits(rect, k)[0]).any(axis=1).sum())
    assert differs >= 1, "ranked by the value the hits are the hits by raw score: the case shows nothing"
    assert sa.last_search_quantity_seconds() > 0


def test_no_quantity_is_the_plain_search(sa, oracle):
    db_seqs, query_seqs, scoring, rect, _ = tie_case(sa, oracle)
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    plain = sa.hip_search(db, queries, scoring, k=33, rect=True)
    same = sa.hip_search(db, queries, scoring, k=33, rect=True, norm=None, pid=None)
    assert len(same) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, same))
    index, value, score, got_rect, vrect = sa.hip_search(db, queries, scoring, k=33, rect=True, values=True)  # norm == NULL in the library
    assert index.tobytes() == plain[0].tobytes() and score.tobytes() == plain[1].tobytes() and value.tobytes() == plain[1].tobytes()
    assert got_rect.tobytes() == plain[2].tobytes() and vrect.tobytes() == plain[2].tobytes()
    assert sa.last_search_quantity_seconds() == 0.0
    # the hits alone, and the rectangles alone
    index, value, score = sa.hip_search(db, queries, scoring, k=7, norm=sa.Norm(LENGTH, MAX))[:3]
    full = sa.hip_search(db, queries, scoring, k=7, rect=True, norm=sa.Norm(LENGTH, MAX))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((index, value, score), full[:3]))
    got_rect, vrect = sa.hip_search(db, queries, scoring, rect=True, pid=COLUMNS)
    assert np.array_equal(got_rect, rect) and np.array_equal(vrect, identity_values(sa, db_seqs, query_seqs, scoring)[COLUMNS])


# ---- 6. batches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["norm", "pid"])
def test_batches_give_the_same_bytes(kind, sa, oracle, monkeypatch):
    db_seqs, query_seqs, scoring, rect, _ = tie_case(sa, oracle)
    n, m, k = len(db_seqs), len(query_seqs), 33
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    quantity = dict(norm=sa.Norm(SELF, MEAN)) if kind == "norm" else dict(pid=DENOMS[1])
    one = sa.hip_search(db, queries, scoring, k=k, rect=True, **quantity)
    assert sa.last_search_breakdown()["batches"] == 1
    per_query = (4 * (n + m) if kind == "norm" else 0) + 8 * n + 20 * k  # (include/seqalign_hip.h: sa_hip_search_norm / _pid)
    monkeypatch.setenv("SA_HIP_SEARCH_BATCH_BYTES", str(12 * per_query))  # 12 queries a batch: 4 batches
    many = sa.hip_search(db, queries, scoring, k=k, rect=True, **quantity)
    bd = sa.last_search_breakdown()
    assert bd["batches"] == 4, bd
    assert sa.last_search_quantity_seconds() > 0 and bd["align"] > 0
    assert len(one) == len(many)
    for a, b in zip(one, many):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(many[3], rect)
