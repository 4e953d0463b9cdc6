"""GPU (-m gpu): the paired diagonal adds of the packed NW kernels (sa_systolic_pk.inc, SA_PK_PAIRED_ADDS: one 64-bit add
for the columns q, q + 1 of a lane, the left neighbour's value in the register below column 0) against the oracle, on the
shapes where the pairing can go wrong: every column count K of a lane (even, odd with its single plain add, K = 1 without
a pair), padding in the first lane, the 16-lane kernels in both forms, frame shifts while the first lane's injected value
sits in the shared left-neighbour register, one-row tiles and a column paired with itself.  Every case checks through
ctx.timing that its columns ran on the packed kernel it aims at.  The no-carry premise of the 64-bit add is guarded by
tests/test_gpu_value_range.py (values at the limits of the u16 fields)."""
import re

import numpy as np
import pytest

from tests.synth import AMINO20, splitmix64

pytestmark = pytest.mark.gpu

BUNDLE = re.compile(r"sa_k_systolic_pk_bundle<nw,(\d+),(\d+),(true|false)>\[K(\d+)-(\d+)\]")


def seq_of(length, seed):
    r = splitmix64(np.arange(length), seed) % np.uint64(20)
    return np.frombuffer(AMINO20, np.uint8)[r.astype(np.int64)].tobytes()


def tri(j):
    return j * (j - 1) // 2


def timed_range(ctx, lo, n):
    import torch
    buf = torch.full((n + 8,), -12345, dtype=torch.int32, device="cuda")
    ctx.timing(True)
    ctx.align_range(lo, n, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tm = ctx.timing_read()
    ctx.timing(False)
    out = buf.cpu().numpy()
    assert (out[n:] == -12345).all(), "wrote past the range"
    return out[:n], tm["kernel"]


def nw(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4)


def check_store(sa, oracle, seqs, lanes, f16=None, columns=True):
    """the whole store against the oracle, then every column as a range of its own: the oracle's scores again, from the
    packed kernel of `lanes`-lane groups whose class list holds the column's K (and of the form f16, where given)"""
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = nw(sa)
    want = oracle.align(store, scoring, triangular=True, threads=8)
    with sa.Context(store, scoring, 0) as ctx:
        got, kernel = timed_range(ctx, 0, store.pairs)
        assert BUNDLE.match(kernel), kernel
        assert np.array_equal(got, want), f"whole store, {kernel}: {np.nonzero(got != want)[0][:8]}"
        for j in range(1, len(seqs) if columns else 1):
            k = (len(seqs[j]) + lanes - 1) // lanes
            got, kernel = timed_range(ctx, tri(j), j)
            mt = BUNDLE.match(kernel)
            assert mt and int(mt[1]) == lanes and int(mt[4]) <= k <= int(mt[5]), f"column {j} ({len(seqs[j])} residues, K {k}) ran on {kernel}"
            if f16 is not None:
                assert (mt[3] == "true") == f16(k), f"column {j} (K {k}) ran on {kernel}"
            assert np.array_equal(got, want[tri(j):tri(j + 1)]), f"column {j} ({len(seqs[j])} residues, K {k}, {kernel})"
    return want


def test_every_column_count_of_the_8_lane_kernels(sa, oracle):
    """48 sequences: every class K = 1 .. 24 at its full width 8 K (no padding) and at 8 K - 7 (seven padding columns in
    the first lane): even and odd K, the single tail add, K = 1"""
    lens = [n for k in range(1, 25) for n in (8 * k - 7, 8 * k)]
    check_store(sa, oracle, [seq_of(n, 100 + i) for i, n in enumerate(lens)], 8, f16=lambda k: True)


def test_16_lane_classes_three_way(sa, oracle):
    """K = 13, 14 (three-way form) and 63, 64 (past SA_PK16_F16_KMAX: two-way form) at 16 K and 16 K - 15, three of each"""
    lens = [n for k in (13, 14, 63, 64) for n in (16 * k - 15, 16 * k)] * 3
    check_store(sa, oracle, [seq_of(n, 200 + i) for i, n in enumerate(sorted(lens))], 16, f16=lambda k: k <= 52)


def test_16_lane_classes_two_way_by_a_short_sequence(sa, oracle):
    """a one-residue sequence in the store: eight frame shifts in flight, K = 13, 14 leave the f16 range and run the
    two-way form of the same adds"""
    lens = [1] + [n for k in (13, 14) for n in (16 * k - 15, 16 * k)] * 3
    seqs = [seq_of(n, 300 + i) for i, n in enumerate(lens)]
    store = sa.SequenceStore.from_sequences(seqs)
    want = oracle.align(store, nw(sa), triangular=True, threads=8)
    with sa.Context(store, nw(sa), 0) as ctx:
        for j in range(1, len(seqs)):
            got, kernel = timed_range(ctx, tri(j), j)
            mt = BUNDLE.match(kernel)
            assert mt and int(mt[1]) == 16 and mt[3] == "false", f"column {j} ({lens[j]} residues) ran on {kernel}"
            assert np.array_equal(got, want[tri(j):tri(j + 1)]), f"column {j} ({lens[j]} residues, {kernel})"
        got, _ = timed_range(ctx, 0, store.pairs)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("no_sort", [False, True])
def test_leader_value_under_frame_shifts(no_sort, sa, oracle, monkeypatch):
    """rows of 1 .. 8 residues in front of columns of about 100: a terminator every 2 .. 9 stream positions, several frame
    shifts in flight while the first lane's injected value sits in the left-neighbour register (which the shift must
    skip for the first lane and apply to the others); arranged streams and store order"""
    monkeypatch.delenv("SA_HIP_NO_SORT", raising=False)
    if no_sort:
        monkeypatch.setenv("SA_HIP_NO_SORT", "1")
    seqs = [seq_of(1 + (i * 5) % 8, 400 + i) for i in range(320)] + [seq_of(n, 500 + n) for n in (97, 100, 100, 104, 105, 112, 100)]
    check_store(sa, oracle, seqs, 8, columns=False)
    store = sa.SequenceStore.from_sequences(seqs)
    with sa.Context(store, nw(sa), 0) as ctx:  # the long columns alone: rows are the short sequences
        want = oracle.align(store, nw(sa), triangular=True, threads=8)
        j = 320
        got, kernel = timed_range(ctx, tri(j), store.pairs - tri(j))
        mt = BUNDLE.match(kernel)
        assert mt and int(mt[1]) == 8, kernel
        assert np.array_equal(got, want[tri(j):])


@pytest.mark.parametrize("length", [8, 100, 112, 185])
def test_one_row_and_a_column_paired_with_itself(length, sa, oracle):
    """K = 1, 13, 14, 24: two sequences (one column, one row: the column is paired with itself), three (one pair; the
    range of its first row alone is one row per column), four (three columns: a pair and a self-paired last one)"""
    for n in (2, 3, 4):
        seqs = [seq_of(length - (i == 0), 600 + length + i) for i in range(n)]
        want = check_store(sa, oracle, seqs, 8)
        if n == 3:
            store = sa.SequenceStore.from_sequences(seqs)
            with sa.Context(store, nw(sa), 0) as ctx:
                got, kernel = timed_range(ctx, 0, 2)  # pairs (0, 1), (0, 2): row 0 of both columns
                assert BUNDLE.match(kernel), kernel
                assert np.array_equal(got, want[:2])
