"""GPU (-m gpu): the packed-u16 and s32 kernels at the LIMITS of their value ranges, against the oracle.

The fast path is exact only because sequencealigner_amd/csrc/sa_limits.cpp admits a class when every live value provably
stays inside the register format: (live + 1) (gain W + slack) + fixed <= limit, where gain W is what a perfect diagonal of
the best-scoring residue earns over all W columns of the class.  Random sequences use a small fraction of that; the inputs
of tests/extremal.py use all of it: homopolymers of the best residue (top), the matrix minimum in every cell and long
gaps (bottom), runs of the shortest sequences behind every long one (as many frame shifts in flight as the bound
assumes), whole tiles of maximal streams (SW's drift).  Every case

  * asks the product's own planner (tests/host_c/limits_sweep.cpp --print: sa_kernel_limits, compiled from the tree) for the
    limits of exactly its store -- nothing of the bound is restated here -- and checks that the store has columns in the
    last admitted class of each form and in the class after it;
  * checks through ctx.timing that those columns ran on the kernel family and form the planner intends (8-lane packed,
    16-lane three-way f16, 16-lane two-way u16, s32), so that a silent fallback cannot turn this into a test of other code;
  * compares np.array_equal with the oracle: arranged row streams, store order (SA_HIP_NO_SORT), ranges that start and end
    inside columns, and the s32 family on the same input (SA_HIP_NO_PK, full 32-sequence streams).

Oracle cost: a full ladder store (about 2 x 10^5 residues, every length twice) is 2 x 10^10 cells; the cases below were sized
with the oracle at 16 threads."""
import numpy as np
import pytest

from tests import extremal as ex
from tests.planner_limits import BUNDLE, PK16_F16_KMAX, PK16_KMAX, PK16_KMIN, PK_KMAX, SYS_CHUNK, class_of, forms, planner  # noqa: F401  (planner: a fixture)

pytestmark = pytest.mark.gpu

# (method, matrix, gaps): the scorings whose last admitted class lies inside the class list for some shortest length --
# 8-lane, 16-lane f16 and 16-lane u16 forms alike -- and nucleotide matrices; each runs the top store, the bottom store
# and a frames store for every shortest length of extremal.SHORTEST
SCORINGS = [
    ("nw", "blosum62", dict(gap_pen=4)),
    ("nw", "blosum62", dict(gap_pen=11)),
    ("nw", "blosum62", dict(gap_pen=20)),
    ("nw", "blosum62", dict(gap_pen=40)),
    ("nw", "pam250", dict(gap_pen=13)),
    ("ga", "blosum62", dict(gap_open=10, gap_extend=1)),
    ("ga", "pam250", dict(gap_open=30, gap_extend=2)),
    ("sw", "blosum62", dict(gap_open=10, gap_extend=1)),
    ("sw", "blosum62", dict(gap_open=12, gap_extend=3)),
    ("sw", "blosum62", dict(gap_open=11, gap_extend=5)),
    ("nw", "nuc44", dict(gap_pen=16)),
    ("ga", "dnafull", dict(gap_open=16, gap_extend=4)),
    ("sw", "nuc44", dict(gap_open=10, gap_extend=1)),
]


def case_id(method, matrix, gaps, m=None):
    return f"{method}-{matrix}-" + "-".join(str(v) for v in gaps.values()) + (f"-m{m}" if m is not None else "")


ROW_CASES = [pytest.param(me, ma, g, id=case_id(me, ma, g)) for me, ma, g in SCORINGS]
FRAME_CASES = [pytest.param(me, ma, g, m, id=case_id(me, ma, g, m)) for me, ma, g in SCORINGS for m in ex.SHORTEST]


def mismatch(got, want, lo=0):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} mismatches, first at packed index {bad[:5] + lo}: got {got[bad[:5]]} want {want[bad[:5]]}"


def device_range(ctx, lo, n):
    import torch
    buf = torch.full((n + 8,), -12345, dtype=torch.int32, device="cuda")
    ctx.align_range(lo, n, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[n:] == -12345).all(), "wrote past the range"
    return out[:n]


def timed_range(ctx, lo, n):
    ctx.timing(True)
    got = device_range(ctx, lo, n)
    tm = ctx.timing_read()
    ctx.timing(False)
    return got, tm["kernel"]


def tri(j):
    return j * (j - 1) // 2


def check_families(ctx, lens, lim, want, tag, only=("pk8", "pk16-f16", "pk16-u16")):
    """the last column of the store in the last admitted class of each form runs on that form, the last column of the class
    after it does not -- each a packed range of its own, timed and compared"""
    for name, g, k, kmax in forms(lim):
        if k == 0 or name not in only:
            continue
        cols = [j for j in range(1, len(lens)) if class_of(lens[j], lim) == (g, k)]
        assert cols, f"{tag}: no column in the last admitted {name} class K = {k}"
        j = cols[-1]
        got, kernel = timed_range(ctx, tri(j), j)
        assert np.array_equal(got, want[tri(j):tri(j + 1)]), f"{tag}: column {j} ({lens[j]} residues, {name} K {k}): " + mismatch(got, want[tri(j):tri(j + 1)], tri(j))
        mt = BUNDLE.match(kernel)
        f16 = name != "pk16-u16" or k <= lim["f16"]
        assert mt and int(mt[1]) == g and (mt[3] == "true") == f16 and int(mt[4]) == k, f"{tag}: {name} K {k} ran on {kernel}"
        if k >= kmax:
            continue
        wide = g * (k + 1)
        cols = [j for j in range(1, len(lens)) if wide - g < lens[j] <= wide]
        assert cols, f"{tag}: no column in the class behind the last admitted {name} class (K = {k + 1})"
        j = cols[-1]
        got, kernel = timed_range(ctx, tri(j), j)
        assert np.array_equal(got, want[tri(j):tri(j + 1)]), f"{tag}: column {j} ({lens[j]} residues, behind {name} K {k}): " + mismatch(got, want[tri(j):tri(j + 1)], tri(j))
        mt = BUNDLE.match(kernel)
        if name == "pk16-f16":  # ... the two-way u16 form of the 16-lane kernels
            assert mt and int(mt[1]) == 16 and mt[3] == "false", f"{tag}: K {k + 1} behind the f16 cut-off ran on {kernel}"
        else:  # (16-lane classes exist only with every 8-lane class: behind an 8-lane boundary nothing is packed)
            assert kernel.startswith("sa_k_systolic<"), f"{tag}: K {k + 1} behind the last {name} class ran on {kernel}"


def run_store(sa, oracle, planner, monkeypatch, seqs, scoring, tag, cuts=4, s32=True):
    """one store through every path; the oracle's matrix is computed once"""
    store = sa.SequenceStore.from_sequences(seqs)
    lens = [len(s) for s in seqs]
    lim = planner(scoring, max(lens), min(lens))
    for name, g, k, kmax in forms(lim):  # the boundary is inside THIS store
        if 0 < k < kmax:
            assert any(class_of(n, lim) == (g, k) for n in lens[1:]), f"{tag}: no column at {name} K = {k}"
            assert any(g * k < n <= g * (k + 1) for n in lens[1:]), f"{tag}: no column at {name} K + 1 = {k + 1}"
    want = oracle.align(store, scoring, triangular=True, threads=16)
    for var in ("SA_HIP_NO_SORT", "SA_HIP_NO_PK", "SA_HIP_CHUNK"):
        monkeypatch.delenv(var, raising=False)
    with sa.Context(store, scoring, 0) as ctx:  # arranged row streams
        got, kernel = timed_range(ctx, 0, store.pairs)
        assert np.array_equal(got, want), f"{tag} limits {lim}, arranged, {kernel}: " + mismatch(got, want)
        packed_store = bool(lim["pk"]) and class_of(max(lens), lim) is not None  # (the longest columns hold most of the cells)
        if packed_store:
            assert "pk_bundle" in kernel, f"{tag}: the longest columns are packed classes, the dominant kernel was {kernel}"
        if lim["pk"]:
            check_families(ctx, lens, lim, want, tag)
        rng = np.random.default_rng(len(seqs))
        for _ in range(cuts):  # both ends inside a column: the two halves of a packed tile carry different row ranges
            j0 = int(rng.integers(store.num // 2, store.num - 2))
            lo = tri(j0) + int(rng.integers(1, j0))
            j1 = min(store.num - 1, j0 + int(rng.integers(1, 12)))
            hi = tri(j1) + int(rng.integers(1, j1))
            got = device_range(ctx, lo, hi - lo)
            assert np.array_equal(got, want[lo:hi]), f"{tag} limits {lim}, range [{lo}, {hi}): " + mismatch(got, want[lo:hi], lo)
    # store order, and streams as long as the planner allows (32 sequences; SW: its chunk cap): a run of shortest sequences
    # then lies inside one stream, not across the streams a small range would be cut into
    monkeypatch.setenv("SA_HIP_NO_SORT", "1")  # (both read when the context is created)
    monkeypatch.setenv("SA_HIP_CHUNK", str(SYS_CHUNK))
    with sa.Context(store, scoring, 0) as ctx:
        got, kernel = timed_range(ctx, 0, store.pairs)
        assert np.array_equal(got, want), f"{tag} limits {lim}, store order, {kernel}: " + mismatch(got, want)
        if packed_store:
            assert "pk_bundle" in kernel, f"{tag}: the longest columns are packed classes, the dominant kernel was {kernel}"
    monkeypatch.delenv("SA_HIP_NO_SORT")
    monkeypatch.delenv("SA_HIP_CHUNK")
    if s32:  # the s32 family on the same input, streams of 32 sequences: the baseline grows by DELTA per sequence
        monkeypatch.setenv("SA_HIP_NO_PK", "1")
        monkeypatch.setenv("SA_HIP_CHUNK", str(SYS_CHUNK))
        with sa.Context(store, scoring, 0) as ctx:
            got, kernel = timed_range(ctx, 0, store.pairs)
            assert lim["sys_ok"] and kernel.startswith("sa_k_systolic<"), f"{tag}: SA_HIP_NO_PK ran {kernel}"
            assert np.array_equal(got, want), f"{tag}, s32 family, {kernel}: " + mismatch(got, want)
        monkeypatch.delenv("SA_HIP_NO_PK")
        monkeypatch.delenv("SA_HIP_CHUNK")
    return lim


def frame_lengths(lim, m):
    """the part of the ladder a frames store keeps: the classes around the last admitted one of each form, the ends of both
    class lists (the longest keeps the store's maximum at 1024, which the limits depend on) and every eighth class --
    what is longer than the shortest sequences m, m + 1"""
    widths = {8, 8 * PK_KMAX, 16 * PK16_KMIN, 16 * PK16_KMAX}
    widths |= {8 * k for k in range(4, PK_KMAX, 8)} | {16 * k for k in range(20, PK16_KMAX, 8)}
    for _, g, k, _ in forms(lim):
        widths |= {g * x for x in (k - 1, k, k + 1) if g * x in ex.CLASS_WIDTHS}
    return [n for n in ex.class_lengths(sorted(widths)) if n > m + 1]


def test_the_boundaries_lie_inside_the_cases(sa, planner):
    """for each of the three forms at least one case has its last admitted class strictly below the form's largest -- a
    condition on the case list (if a fix moves a limit: change the list)"""
    inside = {"pk8": [], "pk16-f16": [], "pk16-u16": []}
    for method, matrix, gaps in SCORINGS:
        scoring = sa.Scoring.from_names(method, matrix, **gaps)
        for m in ex.SHORTEST:
            lim = planner(scoring, ex.MAX_PACKED_LEN, m)
            for name, g, k, kmax in forms(lim):
                if 0 < k < kmax:
                    inside[name].append((case_id(method, matrix, gaps, m), k))
    print(inside)
    assert all(inside.values()), inside


@pytest.mark.parametrize("method,matrix,gaps", ROW_CASES)
def test_top_of_every_class(method, matrix, gaps, sa, oracle, planner, monkeypatch):
    """homopolymers of the best residue at W - 1, W, W + 1 of every class, each length a column behind and a row in front of
    every other: the perfect diagonal over all W columns the bound is made of"""
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    run_store(sa, oracle, planner, monkeypatch, ex.top_store(scoring), scoring, f"top {case_id(method, matrix, gaps)}")


@pytest.mark.parametrize("method,matrix,gaps", ROW_CASES)
def test_bottom_of_every_class(method, matrix, gaps, sa, oracle, planner, monkeypatch):
    """the matrix minimum in every cell of every class, and block sequences whose alignments open one long gap: values at
    the floor of the frame, Gotoh's gap registers and SW's zero decide"""
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    run_store(sa, oracle, planner, monkeypatch, ex.bottom_store(scoring), scoring, f"bottom {case_id(method, matrix, gaps)}")


@pytest.mark.parametrize("method,matrix,gaps,m", FRAME_CASES)
def test_frame_shifts_in_flight(method, matrix, gaps, m, sa, oracle, planner, monkeypatch):
    """top and bottom sequences around the last admitted classes (frame_lengths: NOT the whole ladder -- with a run behind
    each of its 900 sequences the m = 1 store would have 17 000 sequences and the oracle 4 x 10^10 cells per case), each
    followed by a run of 2 live + 2 shortest sequences (m and m + 1 residues, extremal themselves).  In the store-order run
    with 32-sequence streams a long sequence is followed inside its stream by as many terminators as the bound counts,
    unless it sits in the stream's last positions; SW streams are cut at the chunk cap (4 or 8 sequences), so for SW at
    m <= 3 fewer shifts are in flight than the bound allows for -- the bound is then not reached from this side, only
    respected"""
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    lim = planner(scoring, ex.MAX_PACKED_LEN, m)
    seqs = ex.frames_store(scoring, m, frame_lengths(lim, m))
    assert min(map(len, seqs)) == m and max(map(len, seqs)) == ex.MAX_PACKED_LEN
    assert run_store(sa, oracle, planner, monkeypatch, seqs, scoring, f"frames {case_id(method, matrix, gaps, m)}", cuts=3) == lim


@pytest.mark.parametrize("method,gaps", [("nw", dict(gap_pen=4)), ("ga", dict(gap_open=10, gap_extend=1)), ("sw", dict(gap_open=10, gap_extend=1))])
def test_s32_top_at_strip_mined_lengths(method, gaps, sa, oracle, planner, monkeypatch):
    """columns of 1025, 2048 and 3000 best residues (2 and 3 strips) behind a full stream of 1024-residue rows, the s32
    classes with 32-sequence streams: DELTA x stream length at its largest"""
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    best = ex.best_residue(scoring)
    b, c = ex.worst_pair(scoring)
    seqs = [best * 1024] * 44 + [b * 1024] * 10 + [c * 1000] * 10 + [best * n for n in (1025, 2048, 3000)] + [c * 2048] + [best * n for n in (1025, 2048, 3000)]
    store = sa.SequenceStore.from_sequences(seqs)
    lim = planner(scoring, 3000, 1000)
    assert lim["sys_ok"]
    want = oracle.align(store, scoring, triangular=True, threads=16)
    monkeypatch.setenv("SA_HIP_CHUNK", "32")
    for no_pk in (False, True):
        if no_pk:
            monkeypatch.setenv("SA_HIP_NO_PK", "1")
        with sa.Context(store, scoring, 0) as ctx:
            got, kernel = timed_range(ctx, 0, store.pairs)
            assert np.array_equal(got, want), f"{method} no_pk {no_pk} {kernel}: " + mismatch(got, want)
            j = len(seqs) - 1
            got, kernel = timed_range(ctx, tri(j), j)
            assert kernel.endswith("strips>") and np.array_equal(got, want[tri(j):]), kernel


@pytest.mark.parametrize("gap_open,gap_extend", [(12, 3), (11, 5)])
def test_sw_drift_of_the_packed_kernels(gap_open, gap_extend, sa, oracle, planner, monkeypatch):
    """SW's row-shifted domain drifts by |e| per stream position of a tile: a whole tile of `chunk cap` rows of 1024 residues
    per lane group (the longest streams the planner allows this store; four best-residue rows in a stream), against columns
    of the classes around the last admitted ones -- where drift, score and one frame shift together fill the register range
    (|e| = 5: the f16 cut-off lies inside the class list)"""
    scoring = sa.Scoring.from_names("sw", "blosum62", gap_open=gap_open, gap_extend=gap_extend)
    lim = planner(scoring, 1024, 200)
    assert lim["chunk_cap"] == 4 and lim["pk16"] == PK16_KMAX, lim
    if gap_extend == 5:
        assert 0 < lim["f16"] < PK16_F16_KMAX, lim
    widths = [16 * k for k in sorted({lim["f16"] - 1, lim["f16"], lim["f16"] + 1, PK16_F16_KMAX, PK16_F16_KMAX + 1}) if PK16_KMIN <= k]
    seqs = ex.full_stream_store(scoring, 1024, lim["chunk_cap"], columns=ex.class_lengths(widths), seed=gap_extend)
    lens = [len(s) for s in seqs]
    assert planner(scoring, max(lens), min(lens)) == lim
    store = sa.SequenceStore.from_sequences(seqs)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    monkeypatch.setenv("SA_HIP_CHUNK", "32")  # (the cap still holds: streams of exactly `chunk cap` sequences)
    for no_sort in (False, True):
        if no_sort:
            monkeypatch.setenv("SA_HIP_NO_SORT", "1")
        with sa.Context(store, scoring, 0) as ctx:
            got, kernel = timed_range(ctx, 0, store.pairs)
            mt = BUNDLE.match(kernel)
            assert mt and int(mt[1]) == 16, kernel
            assert np.array_equal(got, want), f"|e| {gap_extend} limits {lim} no_sort {no_sort} {kernel}: " + mismatch(got, want)
            check_families(ctx, lens, lim, want, f"sw drift |e| {gap_extend}", only=("pk16-f16", "pk16-u16"))


@pytest.mark.parametrize("gap_extend,admitted", [(16700, True), (16800, False)])
def test_sw_drift_of_the_s32_kernels_at_the_last_admitted_extend(gap_extend, admitted, sa, oracle, planner, monkeypatch):
    """gap_open 2, gap_extend 16700, sequences of 1000 residues: the largest drift SA_SYS_CHUNK (max_len + 1) |e| the planner
    admits to the s32 systolic kernels, in full 32-sequence streams; 16800 is the control that goes to the generic kernels"""
    scoring = sa.Scoring.from_names("sw", "blosum62", gap_open=2, gap_extend=gap_extend)
    lim = planner(scoring, 1000, 1000)
    assert lim["sys_ok"] == int(admitted) and lim["pk"] == 0, lim
    seqs = ex.full_stream_store(scoring, 1000, 32 // 8, seed=7)  # 128 rows: four waves x one 64-lane group x 32
    store = sa.SequenceStore.from_sequences(seqs)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    monkeypatch.setenv("SA_HIP_CHUNK", "32")
    with sa.Context(store, scoring, 0) as ctx:
        got, kernel = timed_range(ctx, 0, store.pairs)
        assert kernel.startswith("sa_k_systolic<") == admitted and "pk_bundle" not in kernel, kernel
        assert np.array_equal(got, want), f"|e| {gap_extend} {kernel}: " + mismatch(got, want)


@pytest.mark.parametrize("method,gaps", [("nw", dict(gap_pen=4)), ("ga", dict(gap_open=10, gap_extend=1)), ("sw", dict(gap_open=10, gap_extend=1))])
def test_int16_exchange_at_its_edge(method, gaps, sa, oracle):
    """the longest sequences for which ctx.scores_fit16 holds: top and bottom pairs of that length through align_range16 +
    widen16; one residue more is refused"""
    import torch
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    best = ex.best_residue(scoring)
    b, c = ex.worst_pair(scoring)

    def fits(n):
        with sa.Context(sa.SequenceStore.from_sequences([best * n, best]), scoring, 0) as ctx:
            return ctx.scores_fit16

    lo, hi = 1, 1 << 16  # fits(lo), not fits(hi)
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    n = lo
    x, y = ex.block_pair(scoring, n // 2)
    seqs = [best * n, best * n, b * n, c * n, best * (n - 1), c * n, b * n, x, y, x, best * n]
    store = sa.SequenceStore.from_sequences(seqs)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    assert np.abs(want).max() <= 32767
    st = torch.cuda.current_stream().cuda_stream
    with sa.Context(store, scoring, 0) as ctx:
        assert ctx.scores_fit16
        b16 = torch.full((store.pairs + 8,), -77, dtype=torch.int16, device="cuda")
        b32 = torch.full((store.pairs + 8,), -77, dtype=torch.int32, device="cuda")
        ctx.align_range16(0, store.pairs, b16.data_ptr(), st)
        ctx.widen16(b16.data_ptr(), b32.data_ptr(), store.pairs, st)
        torch.cuda.synchronize()
        got = b32.cpu().numpy()
        assert (got[store.pairs:] == -77).all() and (b16.cpu().numpy()[store.pairs:] == -77).all()
        assert np.array_equal(got[:store.pairs], want), f"{method} n = {n}: " + mismatch(got[:store.pairs], want)
    with sa.Context(sa.SequenceStore.from_sequences(seqs + [best * (n + 1)]), scoring, 0) as ctx:
        assert not ctx.scores_fit16
        with pytest.raises(sa.AlignError):
            ctx.align_range16(0, 1, b16.data_ptr(), st)
