"""GPU (-m gpu): the pair-per-wave kernels where the 1 GiB budget of their boundary scratch binds, and packed indices across
2^31 in the two of them that unpack an index.

sa_k_pair_per_wave (sa_generic.hip), sa_k_self (sa_normalize.hip), sa_k_trace_fill (sa_traceback.hip) and sa_k_identity
(sa_identity.hip) park the last column of every 64-column strip in a per-wave line of ctx->d_scratch (2 (max_len + 2) ints) and
are launched with at most ctx->generic_blocks workgroups of four waves, which sa_ctx_create sizes as

    max(CUs, min(8 CUs, 2^30 // (32 (max_len + 2))))

(resident_waves_at restates it).  On 256 CUs the budget binds only from 16 383 residues; every other test stays far below
(tests/test_gpu_wave_trips.py says so).  Here one sequence has L = 2^25 // (6 CUs) residues -- 21 845 on 256 CUs, about six
workgroups per CU instead of eight, W' = resident_waves_at(L) = 6140 waves instead of 8192 -- and the assertion W' < 32 CUs is
the evidence that the cap binds: every kernel then takes the generic_blocks branch of its grid sizing as soon as a call holds
more than W' units, the wave stride is not 32 waves per CU, and the lazily allocated payload buffer of sa_k_identity
(generic_blocks * 4 * scratch_stride payloads) depends on the same two numbers.  A kernel launched with one workgroup too many,
or a line one entry too short, would corrupt a neighbour's boundary column and still return plausible numbers.

The store (budget_case): twelve distinct proteins of 1 to 140 residues (63, 64, 65 and 129 among them), repeated in shuffled
order until the triangle holds more than 3 W' pairs (193 sequences, 18 528 pairs at W' = 6140), and one protein of exactly L
residues at the middle index: the column sequence of the lower indices (342 strips), the row sequence of the higher ones --
against the partners of 65 and 129 residues its boundary line is written up to entry L, the last one the line has.  Every call
over the triangle holds more than 2 W' pairs (asserted), and on each of the first three trips more than a quarter of the waves
take a pair with fewer cells than the one before.

Expected values never come from the code under test: oracle.align for every score, oracle.pair(s, s) per distinct sequence for
the self-scores, tests/traceback_ref.py (plain Python over full tables, once per distinct pair of sequences) for identities,
columns, records and CIGARs, Python's // for pid.  The restatement is affordable for every pair of short sequences and for the
long sequence against partners that total 120 residues (1, 2, 5, 17, 30 and 65 residues, in both roles: 5.2 million cells per
method).  For the long sequence's other pairs sa_k_identity is compared with the records of sa_ctx_alignments for the same
pairs: a CROSS-CHECK between two kernels of the library (the other one has tests of its own), not a reference; their scores
are the oracle's all the same.

Order of calls on the one context of a method: score-only range, identity (twice), alignments, self-scores, score-only range
again -- the kernels share d_scratch, and the payload buffer allocated by the first identity call must not disturb it.

Memory: the context's boundary scratch is 1 GiB, the payload buffer 2 GiB; a context is destroyed before the next is made.
Time, measured on a full MI355X (printed at run time): see the figures in the tests' docstrings.

Packed indices across 2^31 (the last test): 65 600 sequences of 1 to 12 residues drawn from 40 distinct ones; the triangle is
never computed.  unpack_pair of sa_k_identity and its twin in sa_k_pair_per_wave take a double-precision square root of
1 + 8 p and correct it; only the packed fast path was checked across 2^31 before.  One range of 300 pairs around 2^31 and
ranges of one pair at 2^31 - 1, 2^31, the first index of column 65 537 and the last pair, (i, j) computed with Python
integers, against traceback_ref and oracle.align_pairs."""
import time

import numpy as np
import pytest
from sequencealigner_amd.binding import ALN_DTYPE

from tests import traceback_ref
from tests.synth import make_protein_set
from tests.tables import GAPS, METHODS
from tests.test_gpu_identity import COLUMNS, MEAN, OUTPUTS, device_identity, packed_pairs, python_pid
from tests.test_gpu_normalize import SELF, device_denominators
from tests.test_gpu_tables import GENERIC, context
from tests.test_gpu_traceback import FIELDS
from tests.test_gpu_value_range import device_range, mismatch
from tests.test_gpu_wave_trips import distinct_pairs, pair_bytes

pytestmark = pytest.mark.gpu

SHORT_LENGTHS = (1, 2, 5, 17, 30, 63, 64, 65, 100, 128, 129, 140)
AFFORDABLE = (1, 2, 5, 17, 30, 65)   # the long sequence's partners with a Python restatement: 120 residues in all


def compute_units() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def resident_waves_at(max_len: int, cus=None) -> int:
    """the waves the pair-per-wave kernels are launched with at most on a context whose longest sequence has max_len residues:
    sa_ctx_create (csrc/sa_context.hip), four waves per workgroup, 32 (max_len + 2) bytes of boundary scratch per workgroup"""
    cus = compute_units() if cus is None else cus
    return 4 * max(cus, min(8 * cus, 2**30 // (32 * (max_len + 2))))


_case = {}


def budget_case(sa):
    """(seqs, store, mid, L, W'), built once"""
    if not _case:
        cus = compute_units()
        length = 2**25 // (6 * cus)
        w = resident_waves_at(length, cus)
        assert cus <= w < 32 * cus == resident_waves_at(200, cus), (cus, length, w)   # the cap binds
        assert sum(AFFORDABLE) == 120 and 65 in AFFORDABLE and set(AFFORDABLE) < set(SHORT_LENGTHS) and {1, 63, 64, 65, 129, 140} <= set(SHORT_LENGTHS)
        distinct = [make_protein_set(1, n, n, 7000 + n)[0] for n in SHORT_LENGTHS]
        assert len(set(distinct)) == 12
        n = 2
        while n * (n - 1) // 2 <= 3 * w:
            n += 1
        rng = np.random.default_rng(61)
        order = np.concatenate([rng.permutation(12) for _ in range((n + 10) // 12)])[:n - 1]   # shuffled, again and again
        mid = n // 2
        assert set(order[:mid].tolist()) == set(order[mid:].tolist()) == set(range(12))   # every partner in both roles
        long_one = make_protein_set(1, length, length, 7999)[0]
        seqs = [distinct[k] for k in order[:mid]] + [long_one] + [distinct[k] for k in order[mid:]]
        store = sa.SequenceStore.from_sequences(seqs)
        assert store.num == n and len(seqs[mid]) == length == store.max and store.pairs > 3 * w and store.pairs > 2 * w
        lens = np.array([len(s) for s in seqs], np.int64)
        ij = np.array(packed_pairs(n), np.int64)
        cells = lens[ij[:, 0]] * lens[ij[:, 1]]
        assert (cells[w:2 * w] < cells[:w]).sum() > w // 4 and (cells[2 * w:3 * w] < cells[w:2 * w]).sum() > w // 4  # a shorter pair after a longer one
        assert (cells[3 * w:] < cells[2 * w:2 * w + len(cells) - 3 * w]).any()
        _case["case"] = (seqs, store, mid, length, w, ij, lens)
        print(f"{cus} CUs: L = {length}, W' = {w} (uncapped {32 * cus}), {n} sequences, {store.pairs} pairs")
    return _case["case"]


_ref, _ref_seconds = {}, {}


def ref_pair(method, scoring, row, col):
    """(the alignment of the pair as (row sequence, column sequence), the same with the caller's a the column sequence) from one
    fill of tests/traceback_ref.py, kept per method and pair of sequences"""
    key = (method, row, col)
    if key not in _ref:
        t0 = time.process_time()
        tabs = traceback_ref.tables(scoring, *traceback_ref.canonical(scoring, row, col, 0, 1))
        _ref[key] = (traceback_ref.align_pair(scoring, row, col, 0, 1, tabs=tabs), traceback_ref.align_pair(scoring, col, row, 1, 0, tabs=tabs))
        _ref_seconds[method] = _ref_seconds.get(method, 0.0) + time.process_time() - t0
    return _ref[key]


_oracle = {}


def oracle_triangle(oracle, method, store, scoring):
    if method not in _oracle:
        _oracle[method] = oracle.align(store, scoring, triangular=True, threads=16)
    return _oracle[method]


def synchronized_seconds(since=None):
    import torch
    torch.cuda.synchronize()
    return time.perf_counter() - (since or 0.0)


# ---- 1. the fallback score kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_fallback_kernel_where_the_cap_binds(method, sa, oracle, monkeypatch):
    """sa_k_pair_per_wave alone (SA_HIP_FORCE_GENERIC) over the whole triangle, against the oracle: one launch of generic_blocks
    workgroups, pairs / launches > 2 W' (18 528 / 1 against 12 280 on 256 CUs).  Device: 19 to 23 ms per method for the kernel."""
    seqs, store, mid, length, w, ij, lens = budget_case(sa)
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    want = oracle_triangle(oracle, method, store, scoring)
    with context(sa, monkeypatch, store, scoring, "SA_HIP_FORCE_GENERIC") as ctx:
        t0 = synchronized_seconds()
        ctx.timing(True)
        got = device_range(ctx, 0, store.pairs)
        tm = ctx.timing_read()
        ctx.timing(False)
        again = device_range(ctx, 0, store.pairs)
        print(f"{method}: {tm}, pairs / launches = {tm['pairs'] / max(tm['launches'], 1):.0f}, 2 W' = {2 * w}; device and copies {synchronized_seconds(t0):.2f} s")
    assert tm["kernel"].startswith(GENERIC), tm
    assert tm["launches"] >= 1 and tm["pairs"] == store.pairs and tm["pairs"] / tm["launches"] > 2 * w, (tm, w)
    assert np.array_equal(got, want), f"{method}, {tm['kernel']}, L = {length}, W' = {w}: " + mismatch(got, want)
    assert np.array_equal(again, got)


# ---- 2 .. 4. identity, self-scores, tracebacks: one context ----------------------------------------------------------------------------
def describe(k, ij, lens, w):
    i, j = ij[k]
    return f"pair {k} = ({i}, {j}), {lens[i]} x {lens[j]} residues, trip {k // w} of wave {k % w}"


@pytest.mark.parametrize("method", METHODS)
def test_identity_tracebacks_and_self_scores_where_the_cap_binds(method, sa, oracle, monkeypatch):
    """sa_k_identity, sa_k_trace_fill with the walk, sa_k_self and the planner's score kernels on one context whose boundary
    scratch is capped (module docstring: the store, the references, the order of calls).  Python restatement: 2 to 5 s of CPU per
    method; device: 2 to 3 s per method, nearly all of it the one wave of sa_k_self that fills L x L cells."""
    seqs, store, mid, length, w, ij, lens = budget_case(sa)
    n, count = store.num, store.pairs
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    scores = oracle_triangle(oracle, method, store, scoring)
    affordable = {s for s in seqs if len(s) in AFFORDABLE}
    assert len(affordable) == len(AFFORDABLE)

    # ---- expected, on the CPU ----
    # identity: every pair of short sequences and the long one against the affordable partners, in both roles
    known = np.zeros(count, bool)
    ident, cols = np.zeros(count, np.int32), np.zeros(count, np.int32)
    for k, (i, j) in enumerate(ij.tolist()):
        if mid in (i, j) and seqs[i + j - mid] not in affordable:
            continue
        ref = ref_pair(method, scoring, seqs[i], seqs[j])[0]
        assert ref["score"] == scores[k], (describe(k, ij, lens, w), ref["score"], scores[k])   # the restatement's scores are the oracle's
        known[k], ident[k], cols[k] = True, ref["identities"], ref["columns"]
    cross = np.flatnonzero(~known)
    assert ((ij[cross] == mid).any(axis=1)).all() and known.sum() == (n - 1) * (n - 2) // 2 + (n - 1 - len(cross))
    roles = {(bool(i == mid), int(lens[i + j - mid])) for i, j in ij[known & (ij == mid).any(axis=1)].tolist()}
    assert roles == {(role, m) for role in (False, True) for m in AFFORDABLE}, roles   # both roles, the partner of 65 residues included
    assert len(cross) >= (n - 1) // 3 and {int(lens[i + j - mid]) for i, j in ij[cross].tolist()} == set(SHORT_LENGTHS) - set(AFFORDABLE)
    pid = np.array([python_pid(int(a), int(c), int(lens[i]), int(lens[j]), COLUMNS) for a, c, (i, j) in zip(ident, cols, ij.tolist())], np.int64).astype(np.int32)

    # tracebacks: 240 distinct ordered pairs of short sequences, the long one with the affordable partners from both sides and in
    # both orders, then repetition (of the short ones) up to 3 W' + 17 pairs
    short_at = np.array([k for k in range(n) if k != mid])
    distinct = short_at[distinct_pairs(n - 1, 240, 7)].astype(np.int32)
    sides = [next(k for k in side if len(seqs[k]) == m) for m in AFFORDABLE for side in (range(mid), range(mid + 1, n))]
    long_pairs = np.array([p for k in sides for p in ((k, mid), (mid, k))], np.int32)
    distinct = np.concatenate([distinct, long_pairs])
    assert len(set(map(tuple, distinct.tolist()))) == len(distinct) == 240 + 24 and (distinct[:, 0] > distinct[:, 1]).sum() > 60
    rng = np.random.default_rng(8)
    pick = np.concatenate([np.arange(len(distinct)), rng.integers(0, 240, 3 * w + 17 - len(distinct))])
    rng.shuffle(pick)
    pairs = distinct[pick]
    assert len(pairs) == 3 * w + 17 and len(pairs) > 2 * w
    rec = np.zeros(len(distinct), ALN_DTYPE)
    runs = []
    for k, (a, b) in enumerate(distinct.tolist()):
        ref = ref_pair(method, scoring, seqs[min(a, b)], seqs[max(a, b)])[a > b]
        for f in FIELDS:
            rec[f][k] = ref[f]
        runs.append(np.array([(run << 4) | "MID".index(op) for run, op in ref["cigar"]], np.uint32))
        rec["cigar_len"][k] = len(runs[-1])
    want = rec[pick]
    want["cigar_off"] = np.cumsum(want["cigar_len"].astype(np.int64)) - want["cigar_len"]
    want_cigar = np.concatenate([runs[k] for k in pick])
    # (the library sorts by scratch size, largest first: the long pairs lead, a wave's later pairs are smaller than its first)
    sizes = np.array([pair_bytes(int(lens[min(a, b)]), int(lens[max(a, b)])) for a, b in pairs.tolist()], np.int64)
    order = np.argsort(-sizes, kind="stable")
    assert (pairs[order[:24]] == mid).any(axis=1).all() and sizes[order[0]] > sizes[order[w]] > sizes[order[2 * w]] >= sizes[order[-1]]
    selfs = {s: oracle.pair(scoring, s, s) for s in set(seqs)}
    want_self = np.array([selfs[s] for s in seqs], np.int32)
    print(f"{method}: {len(_ref)} fills kept, Python restatement of this method {_ref_seconds.get(method, 0.0):.1f} s of CPU")

    # ---- the device: one context, the calls in this order ----
    with context(sa, monkeypatch, store, scoring) as ctx:
        t0 = synchronized_seconds()
        first = device_range(ctx, 0, count)
        assert np.array_equal(first, scores), f"{method} score-only: " + mismatch(first, scores)

        got = device_identity(ctx, 0, count, COLUMNS)
        again = device_identity(ctx, 0, count, COLUMNS)
        t_identity = synchronized_seconds(t0)
        bad = np.flatnonzero(got["score"] != scores)
        assert bad.size == 0, (f"{method}: {bad.size} of {count} scores of sa_k_identity differ, first: {describe(bad[0], ij, lens, w)}: "
                               f"got {got['score'][bad[0]]}, want {scores[bad[0]]}")
        for name, ref in (("identities", ident), ("columns", cols), ("pid", pid)):
            bad = np.flatnonzero(known & (got[name] != ref))
            assert bad.size == 0, (f"{method}: {bad.size} of {known.sum()} {name} differ from the Python restatement, first: {describe(bad[0], ij, lens, w)}, "
                                   f"W' = {w}: got {got[name][bad[0]]}, want {ref[bad[0]]}")
        assert all(again[name].tobytes() == got[name].tobytes() for name in OUTPUTS), f"{method}: a second identity call gives other bytes"

        # the long sequence's other pairs: the cross-check with the device traceback
        alns = ctx.alignments(ij[cross].astype(np.int32))
        for name in ("score", "identities", "columns"):
            bad = np.flatnonzero(got[name][cross] != alns.records[name])
            assert bad.size == 0, (f"{method}: {bad.size} of {len(cross)} {name} differ from sa_ctx_alignments, first: {describe(cross[bad[0]], ij, lens, w)}: "
                                   f"{got[name][cross[bad[0]]]} / {alns.records[name][bad[0]]}")
        cross_pid = np.array([python_pid(int(r["identities"]), int(r["columns"]), int(lens[i]), int(lens[j]), COLUMNS)
                              for r, (i, j) in zip(alns.records, ij[cross].tolist())], np.int64).astype(np.int32)
        assert np.array_equal(got["pid"][cross], cross_pid)
        assert np.array_equal(alns.records["score"], scores[cross])

        # tracebacks on later trips
        t1 = synchronized_seconds()
        traced = ctx.alignments(pairs)
        t_trace = synchronized_seconds(t1)
        assert sa.last_alignments_breakdown()["batches"] == 1
        m_of, n_of = lens[pairs.min(axis=1)], lens[pairs.max(axis=1)]
        for f in FIELDS + ("cigar_len", "cigar_off"):
            bad = np.flatnonzero(traced.records[f] != want[f])
            assert bad.size == 0, (f"{method}: {f} differs for {bad.size} of {len(pairs)} pairs, first: slot {bad[0]}, pair {pairs[bad[0]]}, "
                                   f"{m_of[bad[0]]} x {n_of[bad[0]]} residues, position {int(np.flatnonzero(order == bad[0])[0])} of the sorted list, "
                                   f"W' = {w}: got {traced.records[f][bad[0]]}, want {want[f][bad[0]]}")
        assert np.array_equal(traced.cigar, want_cigar), f"{method}: the flat CIGAR differs"

        # self-scores
        t2 = synchronized_seconds()
        dens = device_denominators(sa, ctx, n, SELF)
        t_self = synchronized_seconds(t2)
        bad = np.flatnonzero(dens != want_self)
        assert bad.size == 0, f"{method}: {bad.size} of {n} self-scores differ, first: sequence {bad[0]} ({lens[bad[0]]} residues): got {dens[bad[0]]}, want {want_self[bad[0]]}"

        # ... and the score-only call again, after the payload buffer came and every kernel used d_scratch
        last = device_range(ctx, 0, count)
        assert np.array_equal(last, scores), f"{method} score-only, after the other calls: " + mismatch(last, scores)
        print(f"{method}: device and copies: score-only + identity twice {t_identity:.2f} s, {len(pairs)} tracebacks {t_trace:.2f} s, self-scores {t_self:.2f} s, "
              f"all calls {synchronized_seconds(t0):.2f} s")


# ---- packed indices across 2^31 ------------------------------------------------------------------------------------------------------------
def unpack(p: int) -> tuple[int, int]:
    """(i, j) of packed index p with Python's integers: the largest j with j (j - 1) / 2 <= p"""
    import math
    j = (1 + math.isqrt(1 + 8 * p)) // 2
    assert j * (j - 1) // 2 <= p < (j + 1) * j // 2
    return p - j * (j - 1) // 2, j


@pytest.mark.parametrize("method", ["nw", "sw"])
def test_packed_indices_across_two_to_the_31(method, sa, oracle, monkeypatch):
    """The context of 65 600 sequences takes under 10 ms to create, the whole case 20 ms: both methods are kept."""
    distinct = [make_protein_set(1, 1 + k % 12, 1 + k % 12, 8000 + k)[0] for k in range(40)]
    assert len(set(distinct)) == 40 and {len(s) for s in distinct} == set(range(1, 13))
    num = 65600
    order = np.random.default_rng(71).integers(0, 40, num)
    seqs = [distinct[k] for k in order]
    store = sa.SequenceStore.from_sequences(seqs)
    lens = [len(s) for s in seqs]
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    assert store.pairs == num * (num - 1) // 2 > 2**31 + 150
    first_of_column = 65537 * 65536 // 2
    ranges = [(2**31 - 150, 300), (2**31 - 1, 1), (2**31, 1), (first_of_column, 1), (store.pairs - 1, 1)]
    assert unpack(first_of_column) == (0, 65537) and unpack(store.pairs - 1) == (num - 2, num - 1) and 2**31 < first_of_column < store.pairs - 1
    assert unpack(2**31 - 1)[1] == unpack(2**31)[1] == 65536
    t0 = time.perf_counter()
    with context(sa, monkeypatch, store, scoring, "SA_HIP_FORCE_GENERIC") as ctx:
        print(f"{method}: context of {num} sequences created in {time.perf_counter() - t0:.2f} s")
        assert ctx.pairs == store.pairs
        for start, count in ranges:
            at = [unpack(p) for p in range(start, start + count)]
            refs = [ref_pair(method, scoring, seqs[i], seqs[j])[0] for i, j in at]
            score = oracle.align_pairs(store, scoring, np.arange(start, start + count, dtype=np.int64))
            assert np.array_equal(score, [r["score"] for r in refs])
            ident = np.array([r["identities"] for r in refs], np.int32)
            cols = np.array([r["columns"] for r in refs], np.int32)
            pid = np.array([python_pid(r["identities"], r["columns"], lens[i], lens[j], MEAN) for r, (i, j) in zip(refs, at)], np.int64).astype(np.int32)
            got = device_identity(ctx, start, count, MEAN)
            for name, ref in (("score", score), ("identities", ident), ("columns", cols), ("pid", pid)):
                bad = np.flatnonzero(got[name] != ref)
                assert bad.size == 0, (f"{method} range [{start}, {start} + {count}): {bad.size} {name} differ, first: packed index {start + bad[0]} = {at[bad[0]]}: "
                                       f"got {got[name][bad[0]]}, want {ref[bad[0]]}")
            ctx.timing(True)
            plain = device_range(ctx, start, count)
            tm = ctx.timing_read()
            ctx.timing(False)
            assert tm["kernel"].startswith(GENERIC) and tm["pairs"] == count, tm
            assert np.array_equal(plain, score), f"{method} sa_k_pair_per_wave, range [{start}, {start} + {count}): " + mismatch(plain, score, start)
            if count == 300:   # one column, 300 rows: a wrong (i, j) is another pair of sequences, and the results tell them apart
                assert len({i for i, _ in at}) == 300 and {j for _, j in at} == {65536}
                assert len(set(score.tolist())) >= 10 and len(set(zip(ident.tolist(), cols.tolist()))) >= 10
