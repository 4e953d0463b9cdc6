"""GPU (-m gpu): the pair-per-wave kernels on the second and third trip of their wavefronts.

sa_k_pair_per_wave (sa_generic.hip), sa_k_self (sa_normalize.hip), sa_k_trace_fill / sa_k_trace_walk and sa_k_trace_compact
(sa_traceback.hip) put one unit of work -- a pair, a sequence -- on one wavefront and run `for (q = wave; q < count; q +=
nwaves)`; the first two include one sweep (sa_wave_sweep.inc) in that loop, the third keeps its own.  They are launched
with at most ctx->generic_blocks workgroups of four waves (the compaction with 2048), which
sa_context.hip sizes at eight workgroups per CU: W = resident_waves() = 8192 on a full MI355X.  A wave starts a second unit
only when a call holds more than W of them, and what then decides the result -- the reset of best / best_r / best_c, h, the
walk's window bounds and the run-length emitter, the boundary scratch line (bndM / bndX) reused by a later unit that is
shorter than the one before, the stride itself -- runs in no other test on purpose.  Every call here holds more than 3 W
units and asserts count > 2 W: that arithmetic is the evidence that every wave made a second and a third trip (in a
partitioned mode W is smaller and the stores shrink with it).

Expected results never come from the code under test: tests/traceback_ref.py (plain Python over full tables) once per
distinct pair, oracle.pair(s, s) once per distinct sequence, oracle.align for the triangle.  Everything is compared exactly
and as whole arrays."""
import numpy as np
import pytest
from sequencealigner_amd.binding import ALN_DTYPE

from tests import traceback_ref
from tests.synth import make_protein_set
from tests.tables import GAPS, METHODS
from tests.test_gpu_normalize import SELF, device_denominators
from tests.test_gpu_tables import GENERIC, context
from tests.test_gpu_traceback import FIELDS, tie_heavy_sequences
from tests.test_gpu_value_range import device_range, mismatch

pytestmark = pytest.mark.gpu


def resident_waves() -> int:
    """W: the waves the pair-per-wave kernels are launched with at most.  Restates sa_ctx_create (csrc/sa_context.hip, "strip-
    boundary scratch of the pair-per-wave kernels"): generic_blocks = 8 workgroups per CU, four waves each.  The 1 GiB budget
    of that scratch (2 (max_len + 2) ints per wave: 1616 bytes at 200 residues, 13 MB for 8192 waves) does not bind for
    sequences of 200 residues or fewer, so every store of this file stays within that length."""
    import torch
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def pair_bytes(m: int, n: int) -> int:
    """sa_tb_pair_bytes (csrc/sa_traceback_core.h): the decision scratch of a pair of m rows and n columns"""
    lines = lambda width: (m + width - 1 + 3) & ~3  # noqa: E731
    strips = (n + 63) >> 6
    return 64 * ((strips - 1) * lines(64) + lines(n - 64 * (strips - 1)))


# ---- tracebacks -------------------------------------------------------------------------------------------------------------------
def trace_store():
    """about 60 sequences of 1 to 140 residues: the strip edges, some of the tie-heavy ones, random proteins"""
    seqs = [s for s in make_protein_set(6, 1, 1, 3)] + [make_protein_set(1, n, n, 40 + n)[0] for n in (63, 64, 65, 128, 129, 140, 2)]
    seqs += [s for s in tie_heavy_sequences() if len(s) > 1]
    seqs += make_protein_set(60 - len(seqs), 3, 140, 5)
    assert len(seqs) == 60 and {1, 63, 64, 65, 128, 129, 140} <= {len(s) for s in seqs} and max(map(len, seqs)) == 140
    return seqs


def distinct_pairs(n: int, count: int, seed: int) -> np.ndarray:
    """`count` distinct ordered pairs (a, b), a != b, in both index orders"""
    rng = np.random.default_rng(seed)
    codes = rng.permutation(n * n)
    codes = codes[codes // n != codes % n][:count]
    return np.stack([codes // n, codes % n], axis=1).astype(np.int32)


def greedy_batches(sizes_sorted, cap):
    """the cut of alignments_impl (sa_traceback.hip): a batch takes pairs while its bytes stay within the cap"""
    counts, filled = [], 0
    for need in sizes_sorted:
        if not counts or filled + need > cap:
            counts.append(0)
            filled = 0
        counts[-1] += 1
        filled += need
    return counts


@pytest.mark.parametrize("method", METHODS)
def test_tracebacks_on_later_trips(method, sa, monkeypatch):
    w = resident_waves()
    seqs = trace_store()
    lens = np.array([len(s) for s in seqs])
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    distinct = distinct_pairs(len(seqs), 240, 7)
    assert len(set(map(tuple, distinct.tolist()))) == 240 and (distinct[:, 0] > distinct[:, 1]).sum() > 60 and (distinct[:, 0] < distinct[:, 1]).sum() > 60
    rng = np.random.default_rng(8)
    pick = np.concatenate([np.arange(240), rng.integers(0, 240, 3 * w + 17 - 240)])   # every distinct pair, then repetition
    rng.shuffle(pick)
    pairs = distinct[pick]
    count = len(pairs)
    assert count == 3 * w + 17 and count > 2 * w

    # expected, from the plain-Python restatement: once per distinct pair, assembled in the caller's order
    rec = np.zeros(240, ALN_DTYPE)
    runs = []
    for k, (a, b) in enumerate(distinct.tolist()):
        ref = traceback_ref.align_pair(scoring, seqs[a], seqs[b], a, b)
        for f in FIELDS:
            rec[f][k] = ref[f]
        runs.append(np.array([(length << 4) | "MID".index(op) for length, op in ref["cigar"]], np.uint32))
        rec["cigar_len"][k] = len(runs[-1])
    want = rec[pick]
    want["cigar_off"] = np.cumsum(want["cigar_len"].astype(np.int64)) - want["cigar_len"]
    want_cigar = np.concatenate([runs[k] for k in pick])
    # the library sorts by scratch size, largest first: a wave's later pairs are smaller than its first, and of other shapes
    m, n = lens[pairs.min(axis=1)], lens[pairs.max(axis=1)]
    sizes = np.array([pair_bytes(int(x), int(y)) for x, y in zip(m, n)], np.int64)
    order = np.argsort(-sizes, kind="stable")
    assert sizes[order[0]] > sizes[order[w]] > sizes[order[2 * w]] and (n[order[:w]] > 64).all() and (n[order[2 * w:3 * w]] <= 64).any()

    def check(got, what):
        for f in FIELDS + ("cigar_len", "cigar_off"):
            bad = np.flatnonzero(got.records[f] != want[f])
            assert bad.size == 0, (f"{method} {what}: {f} differs for {bad.size} of {count} pairs, first: slot {bad[0]}, pair {pairs[bad[0]]}, "
                                   f"{m[bad[0]]} x {n[bad[0]]} residues, position {int(np.flatnonzero(order == bad[0])[0])} of the sorted list, "
                                   f"W = {w}: got {got.records[f][bad[0]]}, want {want[f][bad[0]]}")
        assert np.array_equal(got.cigar, want_cigar), f"{method} {what}: the flat CIGAR differs"

    # batches that each still hold more than W pairs.  Equal shares of the BYTES would not do: the list is sorted by size, so
    # the batch of the largest pairs would hold fewer than W of them.  The cap is what the larger half of the list needs: that
    # half is one batch, the smaller half fits the same cap.
    half = (count + 1) // 2
    cap = int(sizes[order[:half]].sum())
    batches = greedy_batches(sizes[order].tolist(), cap)
    print(f"{method}: W = {w}, {count} pairs, scratch {sizes.sum()} bytes, cap {cap}: batches of {batches} pairs")
    assert len(batches) >= 2 and min(batches) > w and sum(batches) == count, batches

    monkeypatch.delenv("SA_HIP_TRACE_BATCH_BYTES", raising=False)
    with sa.Context(store, scoring) as ctx:
        first = ctx.alignments(pairs)
        assert sa.last_alignments_breakdown()["batches"] == 1
        check(first, "one batch")
        second = ctx.alignments(pairs)
        assert second.records.tobytes() == first.records.tobytes() and second.cigar.tobytes() == first.cigar.tobytes()
    monkeypatch.setenv("SA_HIP_TRACE_BATCH_BYTES", str(cap))
    with sa.Context(store, scoring) as ctx:   # (the switches are read when a context is created)
        cut = ctx.alignments(pairs)
        assert sa.last_alignments_breakdown()["batches"] == len(batches)
    check(cut, f"batches of {batches} pairs")
    assert cut.records.tobytes() == first.records.tobytes() and cut.cigar.tobytes() == first.cigar.tobytes()


# ---- self-scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_self_scores_on_later_trips(method, sa, oracle):
    w = resident_waves()
    lengths = [1, 2, 63, 64, 65, 127, 128, 129, 200] + np.random.default_rng(15).integers(1, 201, 291).tolist()
    distinct = [make_protein_set(1, n, n, 1000 + k)[0] for k, n in enumerate(lengths)]
    assert len(distinct) == 300 and max(map(len, distinct)) == 200
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    selfs = np.array([oracle.pair(scoring, s, s) for s in distinct], np.int32)
    rng = np.random.default_rng(16)
    pick = np.concatenate([np.arange(300), rng.integers(0, 300, 3 * w + 5 - 300)])
    rng.shuffle(pick)
    count = len(pick)
    assert count == 3 * w + 5 and count > 2 * w
    lens = np.array(lengths)[pick]
    assert (lens[w:2 * w] < lens[:w]).sum() > w // 4 and (lens[2 * w:3 * w] < lens[w:2 * w]).sum() > w // 4   # later, shorter units
    store = sa.SequenceStore.from_sequences([distinct[k] for k in pick])
    want = selfs[pick]
    with sa.Context(store, scoring, 0) as ctx:   # only the denominators: the store has 3 x 10^8 pairs
        got = device_denominators(sa, ctx, count, SELF)
        again = device_denominators(sa, ctx, count, SELF)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{method}: {bad.size} of {count} self-scores differ, first: sequence {bad[0]} ({lens[bad[0]]} residues, trip {bad[0] // w} "
                           f"of wave {bad[0] % w}, W = {w}): got {got[bad[0]]}, want {want[bad[0]]}")
    assert np.array_equal(again, got)


# ---- the fallback score kernel ----------------------------------------------------------------------------------------------------
def fallback_store(sa, w):
    n = 2
    while n * (n - 1) // 2 <= 3 * w:   # (223 sequences at W = 8192)
        n += 1
    edges = [1, 2, 63, 64, 65, 127, 128, 129, 200]
    lengths = edges + np.random.default_rng(17).integers(1, 201, n - len(edges)).tolist()
    seqs = [make_protein_set(1, k, k, 2000 + t)[0] for t, k in enumerate(lengths)]
    order = np.random.default_rng(18).permutation(n)
    seqs = [seqs[k] for k in order]
    assert max(map(len, seqs)) == 200 and {64, 65, 128, 129} <= set(map(len, seqs))
    return seqs, sa.SequenceStore.from_sequences(seqs)


def fallback_run(sa, oracle, monkeypatch, method, gaps, switch):
    w = resident_waves()
    seqs, store = fallback_store(sa, w)
    assert store.pairs > 3 * w
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    with context(sa, monkeypatch, store, scoring, switch) as ctx:
        ctx.timing(True)
        got = device_range(ctx, 0, store.pairs)
        tm = ctx.timing_read()
        ctx.timing(False)
        again = device_range(ctx, 0, store.pairs)
    assert tm["kernel"].startswith(GENERIC), tm
    assert tm["launches"] >= 1 and tm["pairs"] == store.pairs and tm["pairs"] / tm["launches"] > 2 * w, tm
    assert np.array_equal(got, want), f"{method} {gaps} {switch}, {tm['kernel']}, W = {w}: " + mismatch(got, want)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("method", METHODS)
def test_fallback_kernel_on_later_trips(method, sa, oracle, monkeypatch):
    fallback_run(sa, oracle, monkeypatch, method, GAPS[method], "SA_HIP_FORCE_GENERIC")


def test_fallback_kernel_on_later_trips_where_the_planner_sends_it(sa, oracle, monkeypatch):
    """Gotoh with |open| < |extend|: no switch, the planner's own choice"""
    fallback_run(sa, oracle, monkeypatch, "ga", dict(gap_open=3, gap_extend=7), None)
