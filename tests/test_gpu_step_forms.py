"""GPU (-m gpu): the chained maxima of the packed NW step (sa_systolic_pk.inc, SA_PK_CHAINED_MAX3: the K dependent
v_pk_maximum3_f16 of a step as asm statements of up to eight links, with no wait state between the links) against the
oracle, where a link that read its neighbour's register too early would show:

  * values at the top of the f16-ordered range: for K = 13 and K = 14 (odd and even pairing of the diagonal adds, statements
    of 8 + 5 and 8 + 6 links) the first NW gap penalty for which the product's own planner (tests/planner_limits.py) makes
    that class the LAST admitted 8-lane class of a store whose shortest sequence has one residue -- four frame shifts in
    flight, homopolymers of the best residue over all W columns, runs of one- and two-residue sequences behind every long
    one (tests/extremal.py: frames_store), arranged streams and store order;
  * every statement length: K = 1 .. 24 are statements of 1 .. 8 links alone, behind one and behind two full ones, with
    top-valued and random columns.

Every case checks through ctx.timing that its columns ran on the packed kernel it aims at.  The oracle's matrix is
computed once per store (a few 10^7 cells)."""
import numpy as np
import pytest

from tests import extremal as ex
from tests.planner_limits import BUNDLE, class_of, planner  # noqa: F401  (planner: a fixture)
from tests.synth import AMINO20, splitmix64

pytestmark = pytest.mark.gpu


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


def seq_of(length, seed):
    r = splitmix64(np.arange(length), seed) % np.uint64(20)
    return np.frombuffer(AMINO20, np.uint8)[r.astype(np.int64)].tobytes()


def columns_on_their_class(ctx, lens, want, ks, tag):
    """the last column of every class K in ks as a range of its own: on the 8-lane NW bundle, in the class K, the oracle's scores"""
    for k in ks:
        cols = [j for j in range(1, len(lens)) if (lens[j] + 7) // 8 == k]
        assert cols, f"{tag}: no column of class K = {k}"
        j = cols[-1]
        got, kernel = timed_range(ctx, tri(j), j)
        mt = BUNDLE.match(kernel)
        assert mt and kernel.startswith("sa_k_systolic_pk_bundle<nw,8,") and mt[3] == "true" and int(mt[4]) == k, f"{tag}: column {j} (K {k}) ran on {kernel}"
        assert np.array_equal(got, want[tri(j):tri(j + 1)]), f"{tag}: column {j} ({lens[j]} residues, K {k}, {kernel})"


@pytest.mark.parametrize("k", [13, 14])
def test_top_values_with_frame_shifts_at_the_last_admitted_class(k, sa, oracle, planner, monkeypatch):
    max_len = 8 * (k + 1) + 1
    found = None
    for gap in range(4, 64):
        scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=gap)
        lim = planner(scoring, max_len, 1)
        if lim["pk"] == k:
            found = scoring, lim, gap
            break
    assert found, f"no gap penalty makes K = {k} the last admitted 8-lane class of a store with a one-residue sequence"
    scoring, lim, gap = found
    seqs = ex.frames_store(scoring, 1, ex.class_lengths([8 * (k - 1), 8 * k, 8 * (k + 1)]), blocks=(4, 20))
    lens = [len(s) for s in seqs]
    assert min(lens) == 1 and max(lens) == max_len and planner(scoring, max(lens), min(lens)) == lim
    assert class_of(8 * k, lim) == (8, k) and class_of(8 * k + 1, lim) is None  # the class behind it is not packed
    store = sa.SequenceStore.from_sequences(seqs)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    for no_sort in (False, True):
        for var in ("SA_HIP_NO_SORT", "SA_HIP_CHUNK", "SA_HIP_NO_PK"):
            monkeypatch.delenv(var, raising=False)
        if no_sort:  # store order, 32-sequence streams: the run of short sequences follows its long one inside a stream
            monkeypatch.setenv("SA_HIP_NO_SORT", "1")
            monkeypatch.setenv("SA_HIP_CHUNK", "32")
        with sa.Context(store, scoring, 0) as ctx:
            got, kernel = timed_range(ctx, 0, store.pairs)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"gap {gap} K {k} no_sort {no_sort} {kernel}: {bad.size} mismatches, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"
            columns_on_their_class(ctx, lens, want, (k - 1, k), f"gap {gap} no_sort {no_sort}")


def test_every_statement_length(sa, oracle):
    """K = 1 .. 24 at 8 K - 7 and 8 K residues: a homopolymer of the best residue twice (a perfect diagonal over all the
    columns of the class) and a random sequence of each length"""
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    best = ex.best_residue(scoring)
    lens = [n for k in range(1, 25) for n in (8 * k - 7, 8 * k)]
    seqs = [best * n for n in lens] + [s for i, n in enumerate(lens) for s in (seq_of(n, 900 + i), best * n)]
    store = sa.SequenceStore.from_sequences(seqs)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    with sa.Context(store, scoring, 0) as ctx:
        got, kernel = timed_range(ctx, 0, store.pairs)
        assert BUNDLE.match(kernel), kernel
        assert np.array_equal(got, want), f"whole store, {kernel}: {np.nonzero(got != want)[0][:8]}"
        columns_on_their_class(ctx, [len(s) for s in seqs], want, range(1, 25), "statement lengths")
