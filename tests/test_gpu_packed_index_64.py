"""GPU (-m gpu): packed indices at and beyond 2^32 on the device.  N = 92 810 sequences, P = 4 306 801 645 pairs: the kernels
that read a finished packed matrix -- sa_k_neighbors, sa_k_edges / the 64-bit scan, the linkage rounds, the radix select, the
normalising sweep, sa_k_expand_full, sa_k_tiles_raw / z_fetch -- and the alignment kernels on ranges beyond 2^32.

The matrix is not aligned: it is generated on the device from tests/synth_triangle.py's closed form value(i, j) (17.2 GB, filled
once), and every expectation comes from that function through (i, j) -- rows of the symmetric matrix from value(min, max), the
planted spanning tree, a two-level 16-bit histogram, torch's floor division over column ranges -- never through the packed
index the kernels compute (tests/test_synth_triangle.py checks that machinery against brute force at small N).  Packed index
2^31 is pair (32 768, 65 536), 2^32 is pair (37 075, 92 682); columns 92 683 .. 92 809 lie wholly beyond 2^32, one full block of
64 columns among them.  A message names the first wrong row or column and on which side of those marks it lies.

The store behind the context is 92 810 sequences of 1 to 12 residues drawn from 40 distinct ones (the pattern of
tests/test_gpu_scratch_budget.py); the last tests align ranges of it beyond 2^32 on every kernel family against the oracle.

Memory: the triangle, and in one test the 34.5 GB full matrix beside it; the fixture asks sa.hip_memory first.  Every output is
allocated one element longer and poisoned.  Tests that overwrite the matrix (the constant fill of the select test, the in-place
normalisation) mark it, and the next reader fills it again.

Time on a full MI355X (profiles/packed_index_64_times.txt; the tests print theirs): the fill 1.0 s, the reference sweep 3.1 s, the
kernels 10 to 110 ms each, the module 25 s.  No reference pass comes near 10 s, so every comparison covers every row and entry.

Tiles: a created job hands its tile rows out in order (sa_zjob_tile_row), so the three tile rows that are compared are reached
by fetching the rows before them too; only the three are copied out of the job's buffer."""
import ctypes as C
import math
import time
import zlib

import numpy as np
import pytest

from tests import synth_triangle as st
from tests.planner_limits import BUNDLE
from tests.synth import make_protein_set
from tests.tables import GAPS

pytestmark = pytest.mark.gpu

N, P = st.N_BIG, st.P_BIG
T_EDGES = 2**30 - 3221225          # the noise passes at about 1e-3
POISON = -0x5A5A5A5B
BLOCK = 512                        # rows of the reference sweep at a time
K_MAX = 64


def region(r: int) -> str:
    return "< 65 536" if r < 65536 else "in [65 536, 92 683)" if r < 92683 else ">= 92 683"


_store = {}


def big_store(sa):
    """(seqs, store) of the N short sequences, built once"""
    if not _store:
        distinct = [make_protein_set(1, 1 + k % 12, 1 + k % 12, 8000 + k)[0] for k in range(40)]
        assert len(set(distinct)) == 40 and {len(s) for s in distinct} == set(range(1, 13))
        order = np.random.default_rng(72).integers(0, 40, N)
        seqs = [distinct[k] for k in order]
        store = sa.SequenceStore.from_sequences(seqs)
        assert store.num == N and store.pairs == P
        _store["case"] = (seqs, store)
    return _store["case"]


def synchronized():
    import torch
    torch.cuda.synchronize()
    return time.perf_counter()


class Big:
    """the context and the generated matrix: buf holds P + 1 elements, buf[P] = buf[0], so that buf[1:] is the same multiset of
    scores behind a pointer that is 4-byte aligned only"""

    def __init__(self, sa, ctx):
        import torch
        self.sa, self.ctx = sa, ctx
        self.buf = torch.empty(P + 1, dtype=torch.int32, device="cuda")
        self.dirty = True
        self.ref = None

    def packed(self):
        """the filled matrix (P elements at a 16-byte aligned address), filled again if a test overwrote it"""
        if self.dirty:
            t0 = synchronized()
            st.fill(self.buf, N)
            self.buf[P] = st.value_int(0, 1)
            print(f"fill of {P} elements: {synchronized() - t0:.2f} s")
            self.dirty = False
            self.spot_check()
        assert self.buf.data_ptr() % 16 == 0
        return self.buf[:P]

    def spot_check(self):
        planted = [st.tri(j) + st.parent(j) for j in (1, 2, 777, 65535, 65536, 65537, 92681, 92682, 92683, 92736, 92799, N - 1)]
        for p in [0, 2**31 - 1, 2**31, 2**32 - 1, 2**32, P - 1, P // 3, 2**32 + 12345] + planted:
            i, j = st.unpack(p)
            assert self.buf[p].item() == st.value_int(i, j), f"the generated matrix at packed index {p} = ({i}, {j})"
        for p in planted:
            assert self.buf[p].item() >= st.PLANT
        assert self.buf[P].item() == self.buf[0].item()


@pytest.fixture(scope="module")
def big(sa):
    import torch
    peak = 4 * (P + 1) + 4 * (N * N + 1) + 24 * 2**30     # the triangle, the full matrix of the expand test, int64 workspace of the references
    if not sa.hip_memory(peak):
        pytest.skip(f"the device has no room for {peak / 2**30:.0f} GiB (and a third more): triangle, full matrix and workspace of N = {N}")
    seqs, store = big_store(sa)
    scoring = sa.Scoring.from_names("nw", "blosum62", **GAPS["nw"])
    t0 = time.perf_counter()
    with sa.Context(store, scoring, 0) as ctx:
        print(f"context of {N} sequences: {time.perf_counter() - t0:.2f} s")
        assert ctx.pairs == P
        case = Big(sa, ctx)
        yield case
        torch.cuda.synchronize()
    case.buf = case.ref = None
    torch.cuda.empty_cache()


def sweep(big):
    """the reference sweep, once: per row the 64 best partners (index, score) and the entries >= T_EDGES (degree, ascending
    columns, scores), from row blocks of value(min, max)"""
    import torch
    if big.ref is None:
        t0 = synchronized()
        index, score, degree, cols, vals = [], [], [], [], []
        for r0 in range(0, N, BLOCK):
            block = st.row_block(r0, min(r0 + BLOCK, N), N, "cuda")
            a, b = st.topk_rows(block, K_MAX)
            index.append(a)
            score.append(b)
            mask = block >= T_EDGES
            degree.append(mask.sum(1))
            cols.append(torch.nonzero(mask)[:, 1].to(torch.int32))
            vals.append(block[mask].to(torch.int32))
        big.ref = dict(index=torch.cat(index), score=torch.cat(score), degree=torch.cat(degree), cols=torch.cat(cols), vals=torch.cat(vals))
        print(f"reference sweep over {N} rows in blocks of {BLOCK}: {synchronized() - t0:.2f} s")
    return big.ref


def first_bad_row(got, want):
    """the first row in which two (rows, k) tensors differ, or None"""
    bad = (got != want).any(1).nonzero()
    return int(bad[0]) if bad.numel() else None


# ---- neighbours -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 5])
def test_neighbors_of_every_row(k, big):
    import torch
    ref = sweep(big)
    d_packed = big.packed()
    d_index = torch.full((N * k + 1,), POISON, dtype=torch.int32, device="cuda")
    d_score = torch.full((N * k + 1,), POISON, dtype=torch.int32, device="cuda")
    t0 = synchronized()
    big.ctx.neighbors(d_packed.data_ptr(), k, d_index.data_ptr(), d_score.data_ptr())
    print(f"neighbours k = {k}: device {1e3 * (synchronized() - t0):.1f} ms")
    assert d_index[-1].item() == POISON and d_score[-1].item() == POISON, "written beyond N * k elements"
    for name, got, want in (("index", d_index, ref["index"]), ("score", d_score, ref["score"])):
        r = first_bad_row(got[:N * k].view(N, k), want[:, :k])
        assert r is None, (f"k = {k}: {name} differs, first in row {r} ({region(r)}): got {got[r * k:r * k + k].tolist()}, "
                           f"want {want[r, :k].tolist()}")


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def test_edges_at_a_threshold(big):
    import torch
    ref = sweep(big)
    want_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(ref["degree"], 0)])
    e = int(want_offsets[-1])
    print(f"T = {T_EDGES}: E = {e}")
    assert 4 * 10**6 < e < 16 * 10**6 and e == ref["cols"].numel() == ref["vals"].numel() and e % 2 == 0    # from the reference alone
    d_packed = big.packed()
    d_offsets = torch.full((N + 2,), POISON, dtype=torch.int64, device="cuda")
    d_index = torch.full((e + 1,), POISON, dtype=torch.int32, device="cuda")
    d_score = torch.full((e + 1,), POISON, dtype=torch.int32, device="cuda")
    t0 = synchronized()
    big.ctx.edge_offsets(d_packed.data_ptr(), T_EDGES, d_offsets.data_ptr())
    t1 = synchronized()
    bad = (d_offsets[:N + 1] != want_offsets).nonzero()
    assert bad.numel() == 0, (f"offsets differ from row {int(bad[0])} ({region(int(bad[0]))}) on: got {d_offsets[int(bad[0])].item()}, "
                              f"want {want_offsets[int(bad[0])].item()}")
    assert d_offsets[N + 1].item() == POISON
    t2 = synchronized()
    big.ctx.edge_fill(d_packed.data_ptr(), T_EDGES, d_offsets.data_ptr(), d_index.data_ptr(), d_score.data_ptr())
    print(f"edges: offsets {1e3 * (t1 - t0):.1f} ms, fill {1e3 * (synchronized() - t2):.1f} ms")
    assert d_index[e].item() == POISON and d_score[e].item() == POISON, "written beyond E elements"
    for name, got, want in (("index", d_index, ref["cols"]), ("score", d_score, ref["vals"])):
        bad = (got[:e] != want).nonzero()
        if bad.numel():
            at = int(bad[0])
            r = int(torch.searchsorted(want_offsets, torch.tensor([at], device="cuda"), right=True)[0]) - 1
            assert False, f"{name} differs at edge {at} of row {r} ({region(r)}): got {got[at].item()}, want {want[at].item()}"


def test_edge_offsets_at_the_lowest_threshold(big):
    """every pair is an edge: offsets[r] = r (N - 1), the last one 8 613 603 290 > 2^33 -- the 64-bit scan without a fill"""
    import torch
    d_packed = big.packed()
    d_offsets = torch.full((N + 2,), POISON, dtype=torch.int64, device="cuda")
    t0 = synchronized()
    big.ctx.edge_offsets(d_packed.data_ptr(), -2**31, d_offsets.data_ptr())
    print(f"edge offsets at INT32_MIN: device {1e3 * (synchronized() - t0):.1f} ms")
    want = torch.arange(N + 1, dtype=torch.int64, device="cuda") * (N - 1)
    assert int(want[-1]) == 8613603290 > 2**33
    bad = (d_offsets[:N + 1] != want).nonzero()
    assert bad.numel() == 0, f"offsets differ from row {int(bad[0])} ({region(int(bad[0]))}) on: got {d_offsets[int(bad[0])].item()}"
    assert d_offsets[N + 1].item() == POISON


# ---- select -----------------------------------------------------------------------------------------------------------------------------
def test_select_ranks_across_the_marks(big):
    import torch
    sa = big.sa
    ranks = [0, P - 1, 2**31 - 1, 2**31, 2**32 - 1, 2**32] + [min(P - 1, int(q * P)) for q in(0.001, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 0.9999)]
    assert len(ranks) == 16 and len(set(ranks)) == 16
    t0 = synchronized()
    want_value, want_below = st.histogram_select(lambda: (v for *_, v in st.slice_values(N, "cuda")), ranks)
    print(f"select: two-level histogram of the closed form {synchronized() - t0:.2f} s")
    assert want_below[0] == 0 and want_value[0] < -2**31 + 64 and want_value[1] == 2**31 - 1 and P - 20000 < want_below[1] < P - 17000   # the extremes
    assert len(set(want_value.tolist())) >= 14 and (np.diff(want_value[np.argsort(ranks)]) >= 0).all()

    def run(view, what):
        d_value = torch.full((17,), POISON, dtype=torch.int32, device="cuda")
        d_below = torch.full((17,), POISON, dtype=torch.int64, device="cuda")
        d_scratch = torch.full((sa.select_scratch_bytes(16),), 0xFF, dtype=torch.uint8, device="cuda")
        t1 = synchronized()
        big.ctx.select(view.data_ptr(), ranks, d_value.data_ptr(), d_below.data_ptr(), d_scratch.data_ptr())
        print(f"select, {what}: device {1e3 * (synchronized() - t1):.1f} ms")
        assert d_value[16].item() == POISON and d_below[16].item() == POISON
        return d_value[:16].cpu().numpy(), d_below[:16].cpu().numpy()

    d_packed = big.packed()
    for view, what in ((d_packed, "16-byte aligned"), (big.buf[1:], "a view offset by 4 bytes")):
        assert view.numel() == P and (view.data_ptr() % 16 == 0) == (what == "16-byte aligned")
        value, below = run(view, what)
        assert value.tolist() == want_value.tolist() and below.tolist() == want_below.tolist(), \
            f"{what}: ranks {ranks}: got {value.tolist()} / {below.tolist()}, want {want_value.tolist()} / {want_below.tolist()}"
    # more than 2^32 entries in one bin of every round
    big.dirty = True
    big.buf.fill_(-123456789)
    value, below = run(big.buf[:P], "one value everywhere")
    assert value.tolist() == [-123456789] * 16 and below.tolist() == [0] * 16, (value.tolist(), below.tolist())


# ---- linkage ----------------------------------------------------------------------------------------------------------------------------
def test_linkage_is_the_planted_tree(big):
    import torch
    sa = big.sa
    t0 = time.perf_counter()
    want_pairs, want_score = st.planted_tree(N)
    print(f"linkage: closed-form tree {time.perf_counter() - t0:.2f} s")
    d_packed = big.packed()
    nbytes = sa.linkage_scratch_bytes(N)
    assert nbytes % 4 == 0
    d_scratch = torch.full((nbytes // 4 + 1,), POISON, dtype=torch.int32, device="cuda")       # dirty
    d_pairs = torch.full((2 * (N - 1) + 1,), POISON, dtype=torch.int32, device="cuda")
    d_score = torch.full((N - 1 + 1,), POISON, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    t1 = synchronized()
    big.ctx.linkage(d_packed.data_ptr(), d_pairs.data_ptr(), d_score.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    print(f"linkage on a stream: device {1e3 * (synchronized() - t1):.1f} ms")
    assert d_pairs[-1].item() == POISON and d_score[-1].item() == POISON and d_scratch[-1].item() == POISON
    pairs, score = d_pairs[:-1].cpu().numpy().reshape(N - 1, 2), d_score[:-1].cpu().numpy()
    bad = np.flatnonzero((pairs != want_pairs).any(1) | (score != want_score))
    assert bad.size == 0, (f"{bad.size} of {N - 1} tree pairs differ, first at place {bad[0]}: got {pairs[bad[0]].tolist()} {score[bad[0]]}, "
                           f"want {want_pairs[bad[0]].tolist()} {want_score[bad[0]]} (column {region(int(want_pairs[bad[0], 1]))})")
    # the host-to-host call over the same matrix tells the rounds
    with sa.DeflateJob(N, 64, d_packed_ptr=d_packed.data_ptr()) as job:
        again = job.linkage()
        rounds = sa.last_linkage_rounds()
    print(f"linkage: {rounds} rounds, {1e3 * sa.last_linkage_seconds():.1f} ms of device time in the host-to-host call")
    assert 1 <= rounds <= math.ceil(math.log2(N)) == 17
    assert np.array_equal(again[0], want_pairs) and np.array_equal(again[1], want_score)


# ---- normalize --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,in_place", [(0, False), (1, False), (2, False), (2, True)])
def test_normalize_every_entry(rule, in_place, big):
    import torch
    sa = big.sa
    assert (sa.NORM_MIN, sa.NORM_MAX, sa.NORM_MEAN) == (0, 1, 2)
    den = st.denominators(N)
    d_den = torch.from_numpy(den).cuda()
    den64 = d_den.to(torch.int64)
    d_packed = big.packed()
    if in_place:
        out = big.buf
        big.dirty = True
    else:
        out = torch.full((P + 1,), POISON, dtype=torch.int32, device="cuda")
    last = out[P].item()
    t0 = synchronized()
    big.ctx.normalize(d_packed.data_ptr(), d_den.data_ptr(), rule, out.data_ptr())
    t1 = synchronized()
    assert out[P].item() == last, "written beyond P elements"
    seen, wrong, count = set(), [], 0
    for j0, j1, i, j, v in st.slice_values(N, "cuda"):
        want = st.normalized(v, den64[i], den64[j], rule).to(torch.int32)
        got = out[st.tri(j0):st.tri(j1)]
        bad = (got != want).nonzero()
        if bad.numel():       # (the first and the last wrong entry of the whole triangle are named: an entry written to the wrong place is wrong twice)
            count += bad.numel()
            for at in sorted({int(bad[0]), int(bad[-1])}) if not wrong else [int(bad[-1])]:
                wrong.append(f"pair ({int(i[at])}, {int(j[at])}) (column {region(int(j[at]))}): got {got[at].item()}, want {want[at].item()}")
        if j1 == N:
            seen = {int(want.min()), int(want.max())}
    assert not wrong, f"rule {rule}, in place {in_place}: {count} entries differ; first " + wrong[0] + "; last " + wrong[-1]
    print(f"normalize rule {rule}{' in place' if in_place else ''}: device {1e3 * (t1 - t0):.1f} ms, floor division over all slices {synchronized() - t1:.2f} s")
    assert -2**31 in seen    # (a denominator <= 0 occurs in the last slice: the undefined ratio is compared too)


# ---- expand_full ------------------------------------------------------------------------------------------------------------------------
def test_expand_full_block_by_block(big):
    import torch
    d_packed = big.packed()
    full = torch.full((N * N + 1,), POISON, dtype=torch.int32, device="cuda")
    t0 = synchronized()
    big.ctx.expand_full(d_packed.data_ptr(), full.data_ptr())
    t1 = synchronized()
    assert full[N * N].item() == POISON, "written beyond N * N elements"
    for r0 in range(0, N, BLOCK):
        r1 = min(r0 + BLOCK, N)
        block = st.row_block(r0, r1, N, "cuda")
        want = torch.where(block == st.DIAGONAL, 0, block).to(torch.int32)
        got = full[r0 * N:r1 * N].view(r1 - r0, N)
        r = first_bad_row(got, want)
        if r is not None:
            c = int((got[r] != want[r]).nonzero()[0])
            assert False, f"row {r0 + r} ({region(r0 + r)}), column {c} ({region(c)}): got {got[r, c].item()}, want {want[r, c].item()}"
    print(f"expand_full: device {1e3 * (t1 - t0):.1f} ms, the rows again and the compare {synchronized() - t1:.2f} s")


# ---- tiles ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 6])
def test_tile_rows_that_hold_the_marks(level, big):
    sa = big.sa
    chunk = 64
    rows = sorted({65536 // chunk, 92682 // chunk, (N - 1) // chunk})
    assert rows == [1024, 1448, 1450]
    d_packed = big.packed()
    t0 = synchronized()
    taken = {}
    with sa.DeflateJob(N, chunk, d_packed_ptr=d_packed.data_ptr(), level=level) as job:
        nc = job.tiles_per_row
        assert nc == (N + chunk - 1) // chunk == rows[-1] + 1
        ptrs, sizes = (C.c_void_p * nc)(), (C.c_size_t * nc)()
        for r in range(rows[-1] + 1):      # in order: the job hands its rows out once, one after the other
            if job._lib.sa_zjob_tile_row(job._h, r, ptrs, sizes):
                raise sa.AlignError(f"tile row {r}")
            if r in rows:
                taken[r] = [C.string_at(ptrs[t], sizes[t]) for t in range(nc)]
    print(f"tiles, level {level}: {rows[-1] + 1} tile rows of {nc} tiles walked in {synchronized() - t0:.2f} s")
    for r in rows:
        r0, r1 = r * chunk, min(r * chunk + chunk, N)
        block = st.row_block(r0, r1, N).numpy()
        want = np.zeros((chunk, nc * chunk), "<i4")
        want[:r1 - r0, :N] = np.where(block == st.DIAGONAL, 0, block)
        for c, z in enumerate(taken[r]):
            raw = z if level == 0 else zlib.decompress(z)
            assert raw == want[:, c * chunk:(c + 1) * chunk].tobytes(), f"level {level}: tile ({r}, {c}), rows from {r0} ({region(r0)}), columns from {c * chunk}"


# ---- alignment ranges beyond 2^32 -------------------------------------------------------------------------------------------------------
RANGES = [(2**32 - 150, 300), (st.tri(92683), 1), (P - 1, 1), (st.tri(N - 2), P - st.tri(N - 2))]
_want = {}


def oracle_ranges(sa, oracle, method):
    if method not in _want:
        seqs, store = big_store(sa)
        scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
        _want[method] = [oracle.align_pairs(store, scoring, np.arange(start, start + count, dtype=np.int64), threads=16) for start, count in RANGES]
    return _want[method]


@pytest.mark.parametrize("switch", [None, "SA_HIP_NO_PK", "SA_HIP_FORCE_GENERIC"])
@pytest.mark.parametrize("method", ["nw", "sw"])
def test_alignment_ranges_beyond_two_to_the_32(method, switch, sa, oracle, monkeypatch):
    from tests.test_gpu_identity import MEAN, device_identity, python_pid
    from tests.test_gpu_scratch_budget import ref_pair
    from tests.test_gpu_tables import GENERIC, S32, context
    from tests.test_gpu_value_range import mismatch, timed_range
    seqs, store = big_store(sa)
    assert st.unpack(RANGES[1][0]) == (0, 92683) and RANGES[3] == (st.tri(N - 2), 2 * N - 3) and RANGES[0][0] + 300 < st.tri(92683)
    assert RANGES[3][0] + RANGES[3][1] == P and all(start + count > 2**32 for start, count in RANGES)
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    want = oracle_ranges(sa, oracle, method)
    t0 = time.perf_counter()
    with context(sa, monkeypatch, store, scoring, switch) as ctx:
        assert ctx.pairs == P
        for (start, count), score in zip(RANGES, want):
            got, kernel = timed_range(ctx, start, count)
            if switch is None:
                assert BUNDLE.match(kernel), f"{method}, range [{start}, +{count}): the default planner ran {kernel}"
            else:
                assert kernel.startswith(S32 if switch == "SA_HIP_NO_PK" else GENERIC), f"{method}, {switch}, range [{start}, +{count}): ran {kernel}"
            assert np.array_equal(got, score), f"{method}, {kernel}, range [{start}, +{count}): " + mismatch(got, score, start)
            if count == 300:    # one column, 300 rows: identities, columns and pid through the unpacking kernel as well
                at = [st.unpack(p) for p in range(start, start + count)]
                assert {j for _, j in at} == {92682} and len({i for i, _ in at}) == 300 and len(set(score.tolist())) >= 10
                refs = [ref_pair(method, scoring, seqs[i], seqs[j])[0] for i, j in at]
                assert np.array_equal(score, [r["score"] for r in refs])
                pid = [python_pid(r["identities"], r["columns"], len(seqs[i]), len(seqs[j]), MEAN) for r, (i, j) in zip(refs, at)]
                dev = device_identity(ctx, start, count, MEAN)
                for name, ref in (("score", score), ("identities", [r["identities"] for r in refs]), ("columns", [r["columns"] for r in refs]), ("pid", pid)):
                    bad = np.flatnonzero(dev[name] != np.array(ref, np.int64).astype(np.int32))
                    assert bad.size == 0, f"{method} {switch}: {bad.size} {name} differ, first: packed index {start + bad[0]} = {at[bad[0]]}: got {dev[name][bad[0]]}, want {ref[bad[0]]}"
    print(f"{method} {switch}: context and four ranges {time.perf_counter() - t0:.2f} s")
