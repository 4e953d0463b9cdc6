"""GPU (-m gpu): normalised scores on the device (sa_ctx_denominators / sa_ctx_normalize / sa_zjob_normalize and the *_norm
one-call variants, csrc/sa_normalize.hip; the tool's --normalize).  Contract (include/seqalign_hip.h): d[k] = the self-score of
sequence k under the context's method and scoring (the table indexed as for any pair) or its length; the score s of (i, j)
becomes floor(s SCALE / D) in parts per million, D = min / max of d[i], d[j] or (2 s SCALE) / (d[i] + d[j]), rounded towards
minus infinity, INT32_MIN for D <= 0, saturated to int32.

The expected answer never comes from the code under test: self-scores are oracle.pair(seq, seq), normalised values are NumPy
int64 floor_divide over the oracle's matrix or a synthetic tensor, and what is selected from them is what the tests of the
neighbours, the graph, the tree and the order statistics expect of any matrix.  Everything is compared exactly."""
import zlib

import numpy as np
import pytest

from tests import tables
from tests.golden_util import tri_to_full
from tests.linkage_ref import prim_tree
from tests.synth import make_near_duplicates, make_protein_set
from tests.test_gpu_edges import assert_same as assert_same_edges, expected_edges, packed_from
from tests.test_gpu_linkage import assert_same as assert_same_tree
from tests.test_gpu_neighbors import assert_same as assert_same_neighbors, expected_neighbors
from tests.test_gpu_select import assert_same as assert_same_select, expected_select, python_rank

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
SCALE = 1000000
POISON = -0x5A5A5A5B
SELF, LENGTH = 0, 1
MIN, MAX, MEAN = 0, 1, 2
AMINO20 = "ARNDCQEGHILKMFPSTWYV"


def normalized(s, di, dj, rule):
    """the contract, with NumPy int64: s, di, dj broadcastable integer arrays"""
    s, di, dj = np.asarray(s, np.int64), np.asarray(di, np.int64), np.asarray(dj, np.int64)
    if rule == MIN:
        den, num = np.minimum(di, dj), s * SCALE
    elif rule == MAX:
        den, num = np.maximum(di, dj), s * SCALE
    else:
        den, num = di + dj, 2 * s * SCALE
    den, num = np.broadcast_arrays(den, num)
    q = np.floor_divide(num, np.where(den > 0, den, 1))
    return np.where(den > 0, np.clip(q, INT32_MIN, INT32_MAX), INT32_MIN).astype(np.int32)


def packed_ij(n):
    """(i, j) of every packed index, from the packed order itself: column j holds i = 0 .. j - 1"""
    j = np.repeat(np.arange(1, n, dtype=np.int64), np.arange(1, n))
    i = np.concatenate([np.arange(c, dtype=np.int64) for c in range(1, n)]) if n > 1 else np.zeros(0, np.int64)
    return i, j


def normalized_full(full, den, rule):
    out = normalized(full, den[:, None], den[None, :], rule)
    np.fill_diagonal(out, 0)
    return out


def device_denominators(sa, ctx, n, source, stream=0):
    import torch
    d = torch.full((n + 64,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.denominators(source, d.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert (got[n:] == POISON).all(), "sa_ctx_denominators wrote beyond N"
    return got[:n].copy()


# ---- 1. the denominators -----------------------------------------------------------------------------------------------------------
SELF_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1025, 2049] + np.random.default_rng(14).integers(20, 191, 60).tolist()


def self_case(sa, method, table, gaps):
    if table == "asym":
        seqs = tables.random_sequences(SELF_LENGTHS, 41)  # all 24 codes
        return seqs, tables.raw_store(sa, seqs), tables.scoring_with(sa, method, gaps, tables.asym())
    seqs = tables.random_sequences(SELF_LENGTHS, 42, AMINO20)
    return seqs, sa.SequenceStore.from_sequences(seqs), sa.Scoring.from_names(method, "blosum62", **gaps)


@pytest.mark.parametrize("table,gaps", [("blosum62", "GAPS"), ("asym", "GAPS"), ("blosum62", "ZERO")])
@pytest.mark.parametrize("method", tables.METHODS)
def test_self_scores_equal_the_oracle_pair_of_a_sequence_with_itself(method, table, gaps, sa, oracle):
    seqs, store, scoring = self_case(sa, method, table, getattr(tables, gaps)[method])
    want = np.array([oracle.pair(scoring, s, s) for s in seqs], np.int32)
    if table == "asym":
        # On the CPU, with the oracle alone.  The score of (a, b) under a table S is the score of (b, a) under its transpose (all
        # three recurrences treat the two gap directions alike), so for a == b the two tables give the SAME self-score: no
        # self-score can tell a transposed lookup from the right one, and none depends on it.  What this case adds over BLOSUM62
        # is a table whose rows and columns differ under every code, B Z X * included; the orientation itself is pinned by
        # the end-to-end cases of tests/test_gpu_tables.py on pairs i != j.
        turned = np.array([oracle.pair(tables.transposed(scoring), s, s) for s in seqs], np.int32)
        cross = [oracle.pair(scoring, seqs[k], seqs[k + 1]) != oracle.pair(tables.transposed(scoring), seqs[k], seqs[k + 1]) for k in range(20, 40)]
        print(f"{method}: {(turned != want).sum()} of {len(seqs)} self-scores differ under the transposed table, {sum(cross)} of 20 pair scores")
        assert np.array_equal(turned, want) and sum(cross) >= 10
    with sa.Context(store, scoring, 0) as ctx:
        got = device_denominators(sa, ctx, store.num, SELF)
        again = device_denominators(sa, ctx, store.num, SELF)
        lengths = device_denominators(sa, ctx, store.num, LENGTH)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{method} {table} {gaps}: {bad.size} self-scores differ, first: sequence {bad[0]} (length {len(seqs[bad[0]])}): got {got[bad[0]]}, want {want[bad[0]]}"
    assert np.array_equal(again, got)
    assert lengths.tolist() == [len(s) for s in seqs] == SELF_LENGTHS


@pytest.mark.parametrize("method", tables.METHODS)
def test_self_scores_equal_the_entry_of_a_sequence_and_its_copy(method, sa):
    """anchored at the kernels pinned to the reference: in a store doubled from 65 to 130 sequences, entry (i, 65 + i) of the
    matrix is sequence i against itself"""
    half = make_protein_set(61, 20, 190, 8) + tables.random_sequences([1, 64, 65, 700], 9, AMINO20)
    assert len(half) == 65
    store = sa.SequenceStore.from_sequences(half + half)
    scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
    full = sa.hip_align(store, scoring, triangular=False)
    with sa.Context(store, scoring, 0) as ctx:
        den = device_denominators(sa, ctx, 130, SELF)
    assert np.array_equal(den[:65], den[65:])
    assert np.array_equal(den[:65], full[np.arange(65), 65 + np.arange(65)])


def test_denominators_refuse_a_source_outside_the_enum(sa):
    import torch
    store = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    d = torch.full((5,), POISON, dtype=torch.int32, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:
        for source in (2, -1):
            with pytest.raises(sa.AlignError, match=f"source {source} is neither"):
                ctx.denominators(source, d.data_ptr())
        with pytest.raises(sa.AlignError, match="null"):
            ctx.denominators(SELF, 0)
        with pytest.raises(sa.AlignError, match="rule 3 is none of"):
            ctx.normalize(d.data_ptr(), d.data_ptr(), 3, d.data_ptr())
        with pytest.raises(sa.AlignError, match="null"):
            ctx.normalize(d.data_ptr(), 0, MIN, d.data_ptr())
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == POISON).all()
        assert device_denominators(sa, ctx, 5, LENGTH).tolist() == store.meta[:, 1].tolist()  # ... and the context goes on working


# ---- 2. the sweep over synthetic tensors ----------------------------------------------------------------------------------------------
def denominator_vectors(n, seed):
    rng = np.random.default_rng(seed)
    mix = np.array([0, -5, 1, 7, SCALE, INT32_MAX, INT32_MIN], np.int32)
    mixed = rng.integers(1, 2001, n).astype(np.int32)
    mixed[rng.permutation(n)[:min(n, 7)]] = rng.permutation(mix)[:min(n, 7)]  # (N >= 7: all seven are there)
    return {"scale": np.full(n, SCALE, np.int32), "ones": np.ones(n, np.int32), "mix": mixed, "random": rng.integers(1, 2001, n).astype(np.int32)}


@pytest.mark.parametrize("n", [2, 3, 17, 65, 700])
def test_sweep_equals_numpy_floor_division(n, sa):
    import torch
    p = n * (n - 1) // 2
    rng = np.random.default_rng(100 + n)
    scores = rng.integers(INT32_MIN, INT32_MAX, p, endpoint=True).astype(np.int32)
    if p >= 3:
        scores[rng.permutation(p)[:2]] = (INT32_MIN, INT32_MAX)
    i, j = packed_ij(n)
    assert i.size == p and (j * (j - 1) // 2 + i == np.arange(p)).all()
    store = sa.SequenceStore.from_sequences(make_protein_set(n, 8, 12, n))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    stream = torch.cuda.Stream()
    tail = 64
    negative_inexact = 0
    with sa.Context(store, scoring, 0) as ctx:
        for name, den in denominator_vectors(n, n).items():
            if n >= 7 and name == "mix":
                assert set([0, -5, 1, 7, SCALE, INT32_MAX, INT32_MIN]) <= set(den.tolist())
            d_den = torch.from_numpy(den).cuda()
            for rule in (MIN, MAX, MEAN):
                want = normalized(scores, den[i], den[j], rule)
                if name == "scale":
                    assert np.array_equal(want, scores)  # identity
                if name == "ones" and rule != MEAN and p >= 3:
                    assert (want == INT32_MAX).any() and (want == INT32_MIN).any()  # saturation
                if True:  # (counted from the expectation alone)
                    dd = np.minimum(den[i], den[j]).astype(np.int64) if rule == MIN else np.maximum(den[i], den[j]).astype(np.int64) if rule == MAX \
                        else den[i].astype(np.int64) + den[j]
                    num = scores.astype(np.int64) * SCALE * (2 if rule == MEAN else 1)
                    negative_inexact += int(((dd > 0) & (num < 0) & (num % np.where(dd > 0, dd, 1) != 0) & (want > INT32_MIN)).sum())
                # out of place on a stream of its own, then in place; 64 elements beyond P keep their poison
                src = torch.cat([torch.from_numpy(scores), torch.full((tail,), POISON, dtype=torch.int32)]).cuda()
                dst = torch.full((p + tail,), POISON, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ctx.normalize(src.data_ptr(), d_den.data_ptr(), rule, dst.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                got, kept = dst.cpu().numpy(), src.cpu().numpy()
                bad = np.flatnonzero(got[:p] != want)
                assert bad.size == 0, (f"N={n} {name} rule {rule}: {bad.size} entries differ, first at {bad[0]} (i {i[bad[0]]}, j {j[bad[0]]}): "
                                       f"s {scores[bad[0]]} d {den[i[bad[0]]]}, {den[j[bad[0]]]}: got {got[bad[0]]}, want {want[bad[0]]}")
                assert (got[p:] == POISON).all() and np.array_equal(kept[:p], scores) and (kept[p:] == POISON).all()
                ctx.normalize(src.data_ptr(), d_den.data_ptr(), rule, src.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                got = src.cpu().numpy()
                assert np.array_equal(got[:p], want) and (got[p:] == POISON).all(), f"N={n} {name} rule {rule}: in place"
                assert np.array_equal(d_den.cpu().numpy(), den)
    if n >= 17:
        print(f"N={n}: {negative_inexact} negative quotients that are no exact multiples")
        # the floor rule is exercised: truncation would miss every one of them by one.  (Scores over all of int32 saturate under
        # small denominators: these are the pairs of the INT32_MAX and SCALE denominators of the mix; the views test below has
        # small scores and a quarter of all entries of this kind.)
        assert negative_inexact >= 4


@pytest.mark.parametrize("shift_in,shift_out", [(1, 1), (1, 0), (3, 2)])
def test_sweep_on_views_off_the_16_byte_alignment(shift_in, shift_out, sa):
    """a tensor one element (and more) off 16-byte alignment, source and destination alike and unlike; in place as well"""
    import torch
    n = 700
    p = n * (n - 1) // 2
    rng = np.random.default_rng(77)
    scores = rng.integers(-50000, 50000, p).astype(np.int32)
    den = rng.integers(1, 2001, n).astype(np.int32)
    i, j = packed_ij(n)
    want = normalized(scores, den[i], den[j], MEAN)
    assert ((want < 0) & ((2 * scores.astype(np.int64) * SCALE) % (den[i].astype(np.int64) + den[j]) != 0)).sum() > p // 4
    store = sa.SequenceStore.from_sequences(make_protein_set(n, 8, 12, n))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    room = p + 64 + 4
    src = torch.full((room,), POISON, dtype=torch.int32, device="cuda")
    dst = torch.full((room,), POISON, dtype=torch.int32, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    src[shift_in:shift_in + p] = torch.from_numpy(scores).cuda()
    d_den = torch.from_numpy(den).cuda()
    torch.cuda.synchronize()
    with sa.Context(store, scoring, 0) as ctx:
        ctx.normalize(src.data_ptr() + 4 * shift_in, d_den.data_ptr(), MEAN, dst.data_ptr() + 4 * shift_out)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[shift_out:shift_out + p], want)
        assert (got[:shift_out] == POISON).all() and (got[shift_out + p:] == POISON).all()
        ctx.normalize(src.data_ptr() + 4 * shift_in, d_den.data_ptr(), MEAN, src.data_ptr() + 4 * shift_in)
        torch.cuda.synchronize()
        got = src.cpu().numpy()
        assert np.array_equal(got[shift_in:shift_in + p], want)
        assert (got[:shift_in] == POISON).all() and (got[shift_in + p:] == POISON).all()


# ---- 3. end to end: what is selected from normalised scores, against the oracle's matrix normalised in NumPy ---------------------------
N_E2E = 700
_e2e = {}


def e2e_case(sa, oracle, method):
    """store, scoring, the oracle's raw full matrix and the oracle's self-scores of 700 proteins of mixed lengths with near
    duplicates (computed once per method)"""
    if method not in _e2e:
        seqs = make_near_duplicates(make_protein_set(N_E2E, 20, 190, 61), 0.3, 0.1, 61)
        store = sa.SequenceStore.from_sequences(seqs)
        scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
        full = tri_to_full(oracle.align(store, scoring, triangular=True), N_E2E)
        selfs = np.array([oracle.pair(scoring, s, s) for s in seqs], np.int32)
        lengths = np.array([len(s) for s in seqs], np.int32)
        _e2e[method] = (store, scoring, full, selfs, lengths)
    return _e2e[method]


@pytest.mark.parametrize("method,source,rule", [("nw", SELF, MIN), ("ga", SELF, MIN), ("sw", SELF, MIN), ("sw", LENGTH, MAX)])
def test_selections_over_normalised_scores(method, source, rule, sa, oracle):
    store, scoring, raw, selfs, lengths = e2e_case(sa, oracle, method)
    n = N_E2E
    den = selfs if source == SELF else lengths
    full = normalized_full(raw, den, rule)
    norm = sa.Norm(source, rule)
    what = f"{method} source {source} rule {rule}"
    with sa.Context(store, scoring, 0) as ctx:
        assert np.array_equal(device_denominators(sa, ctx, n, source), den)

    # neighbours: the lexsort of the normalised matrix; and the lists do differ from the raw ones (from the oracle alone)
    differ = differ_got = 0
    for k in (1, 8, 64):
        want, want_raw = expected_neighbors(full, k), expected_neighbors(raw, k)
        differ += int((want[0] != want_raw[0]).any(axis=1).sum())
        index, score, got_den = sa.hip_neighbors(store, scoring, k, norm=norm)
        assert_same_neighbors((index, score), want, f"{what} k={k}")
        assert got_den.dtype == np.int32 and np.array_equal(got_den, den)
        plain = sa.hip_neighbors(store, scoring, k)
        assert_same_neighbors(plain, want_raw, f"{what} k={k} raw")
        differ_got += int((plain[0] != index).any(axis=1).sum())
    assert differ >= 1 and differ_got == differ  # normalised and raw neighbour lists are not the same lists
    assert sa.last_normalize_seconds() > 0.0

    # the graph at the 0.95 quantile of the normalised values
    tri = np.sort(packed_from(full))
    p = tri.size
    t = int(tri[python_rank(p, 0.95)])
    want = expected_edges(full, t)
    assert 0 < want[0][-1] < n * (n - 1)
    offsets, index, score, got_den = sa.hip_edges(store, scoring, t, norm=norm)
    assert_same_edges((offsets, index, score), want, what)
    assert np.array_equal(got_den, den)

    # the tree
    want_tree = prim_tree(full)
    pairs, score, got_den = sa.hip_linkage(store, scoring, norm=norm)
    assert_same_tree((pairs, score), want_tree, what)
    assert np.array_equal(got_den, den)

    # order statistics, alone and as the cut of the graph and beside the tree
    ranks = [0, p - 1, p // 2, python_rank(p, 0.95), python_rank(p, 0.99)]
    want_sel = expected_select(tri, ranks)
    value, below, got_den = sa.hip_select(store, scoring, ranks, norm=norm)
    assert_same_select((value, below), want_sel, what)
    assert np.array_equal(got_den, den)
    offsets, index, score, cut, under, got_den = sa.hip_edges_at_rank(store, scoring, python_rank(p, 0.95), norm=norm)
    assert cut == t and under == int(np.searchsorted(tri, t, "left"))
    assert_same_edges((offsets, index, score), want, f"{what} at rank")
    assert np.array_equal(got_den, den)
    pairs, score, value, below, got_den = sa.hip_linkage_with_ranks(store, scoring, ranks, norm=norm)
    assert_same_tree((pairs, score), want_tree, f"{what} with ranks")
    assert_same_select((value, below), want_sel, f"{what} with ranks")
    assert np.array_equal(got_den, den)


def test_no_norm_is_the_plain_call(sa, oracle):
    """norm=None: two results, the bytes of the call without the keyword (which the suites of the four features pin to the oracle)"""
    store, scoring, raw, _, _ = e2e_case(sa, oracle, "nw")
    tri = np.sort(packed_from(raw))
    p = tri.size
    lib = sa.load_library()
    import ctypes as C
    n, k = N_E2E, 8
    sc, inp = scoring._as_c(), store._as_c()
    index, score = np.full((2, n * k), POISON, np.int32), np.full((2, n * k), POISON, np.int32)
    assert lib.sa_hip_neighbors(inp, C.byref(sc), k, index[0].ctypes.data, score[0].ctypes.data)
    assert lib.sa_hip_neighbors_norm(inp, C.byref(sc), k, index[1].ctypes.data, score[1].ctypes.data, None)
    assert index[0].tobytes() == index[1].tobytes() and score[0].tobytes() == score[1].tobytes()
    assert_same_neighbors((index[0].reshape(n, k), score[0].reshape(n, k)), expected_neighbors(raw, k), "norm == NULL")
    from sequencealigner_amd.binding import _take_edges, _take_linkage
    t = int(tri[python_rank(p, 0.99)])
    a, b = _take_edges(lib, lib.sa_hip_edges(inp, C.byref(sc), t)), _take_edges(lib, lib.sa_hip_edges_norm(inp, C.byref(sc), t, None))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0][-1] > 0
    a, b = _take_linkage(lib, lib.sa_hip_linkage(inp, C.byref(sc))), _take_linkage(lib, lib.sa_hip_linkage_norm(inp, C.byref(sc), None))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    ranks = np.array([0, p // 2, p - 1], np.int64)
    value, below = np.full((2, 3), POISON, np.int32), np.full((2, 3), POISON, np.int64)
    assert lib.sa_hip_select(inp, C.byref(sc), ranks.ctypes.data, 3, value[0].ctypes.data, below[0].ctypes.data)
    assert lib.sa_hip_select_norm(inp, C.byref(sc), ranks.ctypes.data, 3, value[1].ctypes.data, below[1].ctypes.data, None)
    assert value[0].tobytes() == value[1].tobytes() and below[0].tobytes() == below[1].tobytes()
    assert_same_select((value[0], below[0]), expected_select(tri, ranks), "norm == NULL")
    assert len(sa.hip_neighbors(store, scoring, k, norm=None)) == 2 and len(sa.hip_select(store, scoring, [0], norm=None)) == 2


def test_a_bad_norm_is_refused_before_the_alignment_and_the_process_lives_on(sa, oracle):
    store, scoring, raw, selfs, _ = e2e_case(sa, oracle, "nw")
    with pytest.raises(sa.AlignError, match="source 7 is neither"):
        sa.hip_linkage(store, scoring, norm=sa.Norm(7, MIN))
    with pytest.raises(sa.AlignError, match="rule 9 is none of"):
        sa.hip_neighbors(store, scoring, 3, norm=sa.Norm(SELF, 9))
    index, score, den = sa.hip_neighbors(store, scoring, 3, norm=sa.Norm(SELF, MEAN))
    assert_same_neighbors((index, score), expected_neighbors(normalized_full(raw, selfs, MEAN), 3), "after the refusals")


# ---- 4. the tile job -----------------------------------------------------------------------------------------------------------------
N_JOB, CHUNK = 300, 64
_job = {}


def job_case(sa, oracle):
    if not _job:
        seqs = make_near_duplicates(make_protein_set(N_JOB, 20, 120, 62), 0.3, 0.1, 62)
        store = sa.SequenceStore.from_sequences(seqs)
        scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
        raw = tri_to_full(oracle.align(store, scoring, triangular=True), N_JOB)
        selfs = np.array([oracle.pair(scoring, s, s) for s in seqs], np.int32)
        _job["case"] = (seqs, store, scoring, raw, selfs)
    return _job["case"]


def test_tile_job_normalize(sa, oracle, monkeypatch):
    import torch
    seqs, store, scoring, raw, selfs = job_case(sa, oracle)
    n = N_JOB
    norm = sa.Norm(SELF, MIN)
    full = normalized_full(raw, selfs, MIN)
    tri = np.sort(packed_from(full))
    p = tri.size
    nc = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((nc * CHUNK, nc * CHUNK), np.int32)
    pad[:n, :n] = raw
    ranks = [0, p // 2, python_rank(p, 0.9), p - 1]
    t = int(tri[python_rank(p, 0.9)])
    with sa.DeflateJob.begin(store, scoring, CHUNK, level=1) as job:
        with pytest.raises(sa.AlignError) as early:
            job.normalize(norm)  # the walk has not ended: the tiles still to come must be raw
        with pytest.raises(sa.AlignError) as early_edges:
            job.edges(0)
        assert "not finished" in str(early.value)
        assert str(early.value).replace("sa_zjob_normalize", "sa_zjob_edges") == str(early_edges.value)  # the same wording
        tiles = 0
        while True:  # ... and the job goes on working: every tile inflates to the RAW matrix
            batch = job.next()
            if not batch:
                break
            for r, c, z in batch:
                assert zlib.decompress(z) == pad[r * CHUNK:(r + 1) * CHUNK, c * CHUNK:(c + 1) * CHUNK].astype("<i4").tobytes(), (r, c)
                tiles += 1
        assert tiles == nc * nc
        assert_same_neighbors(job.neighbors(5), expected_neighbors(raw, 5), "before normalize: raw")
        with pytest.raises(sa.AlignError, match="source 5 is neither"):
            job.normalize(sa.Norm(5, MIN))
        den = job.normalize(norm)
        assert den.dtype == np.int32 and np.array_equal(den, selfs)
        assert sa.last_normalize_seconds() > 0.0
        assert_same_neighbors(job.neighbors(5), expected_neighbors(full, 5), "tile job")
        assert_same_edges(job.edges(t), expected_edges(full, t), "tile job")
        assert_same_tree(job.linkage(), prim_tree(full), "tile job")
        assert_same_select(job.select(ranks), expected_select(tri, ranks), "tile job")
        with pytest.raises(sa.AlignError, match="normalised already"):
            job.normalize(norm)
        assert_same_select(job.select(ranks), expected_select(tri, ranks), "after the refused second call")
    # a job over the caller's matrix: const, not the job's to rewrite
    d_packed = torch.from_numpy(packed_from(raw)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, CHUNK, d_packed_ptr=d_packed.data_ptr(), level=1) as job:
        with pytest.raises(sa.AlignError, match="caller's matrix"):
            job.normalize(norm)
        assert_same_neighbors(job.neighbors(5), expected_neighbors(raw, 5), "created job")
    assert np.array_equal(d_packed.cpu().numpy(), packed_from(raw))
    monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
    with sa.DeflateJob.begin(store, scoring, CHUNK, level=1) as job:
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="dealt over 3 jobs"):
            job.normalize(norm)


# ---- 5. the tool -----------------------------------------------------------------------------------------------------------------------
def test_cli_normalize(tmp_path, sa, oracle):
    from tests.host_binding import h5_matrix, h5_sequences
    from tests.test_edges_host import EDGE_SETS, h5_array, h5_edges
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_linkage_host import TREE_SETS, h5_linkage
    from tests.test_neighbors_host import h5_dataset, h5_names
    from tests.test_normalize_host import NORM_SETS
    from tests.test_select_host import QUANTILE_SETS
    seqs, store, scoring, raw, selfs = job_case(sa, oracle)
    n = N_JOB
    norm = sa.Norm(SELF, MIN)
    full = normalized_full(raw, selfs, MIN)
    tri = np.sort(packed_from(full))
    p = tri.size
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]
    fractions = [0.9, 0.5, 0.99]  # --min-quantile first, then --quantiles
    ranks = [python_rank(p, q) for q in fractions]
    t = int(tri[ranks[0]])
    # the binding's normalised results (pinned to NumPy above), and NumPy's again
    nb = sa.hip_neighbors(store, scoring, 5, norm=norm)[:2]
    assert_same_neighbors(nb, expected_neighbors(full, 5), "binding")
    eg = sa.hip_edges(store, scoring, t, norm=norm)[:3]
    assert_same_edges(eg, expected_edges(full, t), "binding")
    tree = sa.hip_linkage(store, scoring, norm=norm)[:2]
    assert_same_tree(tree, prim_tree(full), "binding")

    def normalization_sets(path):
        assert np.array_equal(h5_array(path, "normalization_denominators", "<i4"), selfs)
        assert h5_array(path, "normalization_rule", "<i4").tolist() == [SELF, MIN]
        assert h5_array(path, "normalization_scale", "<i4").tolist() == [SCALE]

    def quantile_sets(path, fr):
        assert h5_array(path, "score_quantiles", "<f8").tolist() == fr
        assert_same_select((h5_array(path, "score_quantile_values", "<i4"), h5_array(path, "score_quantile_below", "<i8")),
                           expected_select(tri, [python_rank(p, q) for q in fr]), str(path))

    def everything(path):
        assert h5_names(path) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores", *EDGE_SETS, *TREE_SETS,
                                  *QUANTILE_SETS, "/edge_min_score", *NORM_SETS}
        assert np.array_equal(h5_matrix(path, n), raw)  # the matrix stays raw
        assert h5_sequences(path) == seqs
        assert_same_neighbors((h5_dataset(path, "neighbor_indices", (n, 5)), h5_dataset(path, "neighbor_scores", (n, 5))), nb, str(path))
        assert_same_edges(h5_edges(path, n), eg, str(path))
        assert h5_array(path, "edge_min_score", "<i4").tolist() == [t]
        assert_same_tree(h5_linkage(path, n), tree, str(path))
        quantile_sets(path, fractions)
        normalization_sets(path)

    options = ["--normalize", "self-min", "-k", 5, "--min-quantile", 0.9, "--linkage", "--quantiles", "0.5,0.99"]
    out = tmp_path / "all.h5"
    res = run("-i", fasta, "-o", out, *flags, *options, "-B", "-V")
    assert "Normalisation on the device, self-min" in res.stdout and "Scores normalised in place on the device" in res.stdout, res.stdout
    assert "second alignment pass" not in res.stdout, res.stdout
    everything(out)
    # the paths that keep no device matrix: second passes, through the *_norm calls
    hostm = tmp_path / "hostm.h5"
    res = run("-i", fasta, "-o", hostm, *flags, *options, "-B", "-V", env={"SA_HOST_MATRIX": "1"})
    assert "second alignment pass" in res.stdout and "Normalisation on the device" in res.stdout, res.stdout
    everything(hostm)
    # the matrix never leaves the device
    only = tmp_path / "nb_only.h5"
    run("-i", fasta, "-o", only, *flags, "--normalize", "self-min", "-k", 5, "--neighbors-only", "-Q")
    assert h5_names(only) == {"/sequences", "/neighbor_indices", "/neighbor_scores", *NORM_SETS}
    assert_same_neighbors((h5_dataset(only, "neighbor_indices", (n, 5)), h5_dataset(only, "neighbor_scores", (n, 5))), nb, "neighbors-only")
    normalization_sets(only)
    only = tmp_path / "eg_only.h5"
    run("-i", fasta, "-o", only, *flags, "--normalize=self-min", "--min-quantile", 0.9, "--edges-only", "-Q")
    assert h5_names(only) == {"/sequences", *EDGE_SETS, *QUANTILE_SETS, "/edge_min_score", *NORM_SETS}
    assert_same_edges(h5_edges(only, n), eg, "edges-only")
    quantile_sets(only, [0.9])
    normalization_sets(only)
    only = tmp_path / "eg_score_only.h5"
    run("-i", fasta, "-o", only, *flags, "--normalize", "self-min", "--min-score", t, "--edges-only", "-Q")  # T in parts per million
    assert_same_edges(h5_edges(only, n), eg, "edges-only at a given T")
    only = tmp_path / "lk_only.h5"
    run("-i", fasta, "-o", only, *flags, "--normalize", "self-min", "--linkage-only", "--clusters", t, "--quantiles", "0.5,0.99", "-Q")
    assert h5_names(only) == {"/sequences", *TREE_SETS, "/cluster_labels", *QUANTILE_SETS, *NORM_SETS}
    assert_same_tree(h5_linkage(only, n), tree, "linkage-only")
    from tests.linkage_ref import labels_at
    assert np.array_equal(h5_array(only, "cluster_labels", "<i4"), labels_at(full, t)[0])
    quantile_sets(only, [0.5, 0.99])
    normalization_sets(only)
    # without --normalize: none of the three datasets, and raw selections
    plain = tmp_path / "plain.h5"
    run("-i", fasta, "-o", plain, *flags, "-k", 5, "--linkage", "-Q")
    assert h5_names(plain) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores", *TREE_SETS}
    assert_same_neighbors((h5_dataset(plain, "neighbor_indices", (n, 5)), h5_dataset(plain, "neighbor_scores", (n, 5))),
                          expected_neighbors(raw, 5), "plain")
    # len-mean through the tool: the lengths are the denominators
    lens = tmp_path / "len.h5"
    run("-i", fasta, "-o", lens, *flags, "--normalize", "len-mean", "-k", 5, "--neighbors-only", "-Q")
    lengths = np.array([len(s) for s in seqs], np.int32)
    assert np.array_equal(h5_array(lens, "normalization_denominators", "<i4"), lengths)
    assert h5_array(lens, "normalization_rule", "<i4").tolist() == [LENGTH, MEAN]
    assert_same_neighbors((h5_dataset(lens, "neighbor_indices", (n, 5)), h5_dataset(lens, "neighbor_scores", (n, 5))),
                          expected_neighbors(normalized_full(raw, lengths, MEAN), 5), "len-mean")
