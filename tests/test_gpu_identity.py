"""GPU (-m gpu): percent identity of every pair on the device (sa_ctx_identity_range / sa_hip_identity / sa_zjob_identity and the
*_pid one-call selections, csrc/sa_identity.hip; the tool's --identity).  Contract (include/seqalign_hip.h): identities and
columns of the ONE canonical alignment the tie rule of "alignments for chosen pairs" fixes, carried forward through the sweep;
pid = floor(identities SCALE / D) in parts per million, INT32_MIN for D <= 0.

The expected answer never comes from the code under test: scores are the oracle's, identities and columns come from
tests/traceback_ref.py (plain Python over full tables), pid is Python's //, selections are NumPy's.  Everything is compared
exactly.

1. contract: every scoring of the traceback contract test + an asymmetric table, whole arrays, all four denominators
2. strips: lengths around the 64-column strips, default gaps and gaps of 0
3. later trips: more than 2 W pairs, a short pair after a long one on the same wavefront
4. ranges: a range that begins and ends mid-column, any subset of the outputs, pid in place over scores
5. device against device: the records of sa_ctx_alignments for 44 850 pairs
6. selections over pid, the tool, the tile job"""
import numpy as np
import pytest

from tests import tables, traceback_ref
from tests.golden_util import tri_to_full
from tests.linkage_ref import labels_at, prim_tree
from tests.synth import make_near_duplicates, make_protein_set
from tests.test_gpu_edges import assert_same as assert_same_edges, expected_edges
from tests.test_gpu_linkage import assert_same as assert_same_tree
from tests.test_gpu_neighbors import assert_same as assert_same_neighbors, expected_neighbors
from tests.test_gpu_select import assert_same as assert_same_select, expected_select
from tests.test_gpu_traceback import CONTRACT_SCORINGS, tie_heavy_sequences
from tests.test_gpu_wave_trips import resident_waves

pytestmark = pytest.mark.gpu

INT32_MIN = -2**31
SCALE = 1000000
POISON = -0x5A5A5A5B
COLUMNS, SHORTER, LONGER, MEAN = 0, 1, 2, 3
DENOMS = (COLUMNS, SHORTER, LONGER, MEAN)
OUTPUTS = ("score", "identities", "columns", "pid")


def python_pid(identities: int, columns: int, li: int, lj: int, denom: int) -> int:
    """the contract, with Python's integers"""
    den, num = {COLUMNS: (columns, identities * SCALE), SHORTER: (min(li, lj), identities * SCALE), LONGER: (max(li, lj), identities * SCALE),
                MEAN: (li + lj, 2 * identities * SCALE)}[denom]
    return INT32_MIN if den <= 0 else num // den


def packed_pairs(n):
    """(i, j) of every packed index: column j holds i = 0 .. j - 1"""
    return [(i, j) for j in range(1, n) for i in range(j)]


def reference(scoring, seqs, pairs, flipped=False, cache=None):
    """(score, identities, columns) int32 arrays of the pairs (i < j) from tests/traceback_ref.py; with `flipped` also the share
    of pairs whose (identities, columns) change under the other tie order.  `cache`: keyed by the two sequences' bytes."""
    out = np.zeros((3, len(pairs)), np.int32)
    changed = 0
    for t, (i, j) in enumerate(pairs):
        key = (seqs[i], seqs[j])
        if cache is not None and key in cache:
            out[:, t] = cache[key]
            continue
        lo, hi = traceback_ref.canonical(scoring, seqs[i], seqs[j], i, j)
        tabs = traceback_ref.tables(scoring, lo, hi)
        ref = traceback_ref.align_pair(scoring, seqs[i], seqs[j], i, j, tabs=tabs)
        out[:, t] = (ref["score"], ref["identities"], ref["columns"])
        if flipped:
            other = traceback_ref.align_pair(scoring, seqs[i], seqs[j], i, j, flipped_ties=True, tabs=tabs)
            changed += (other["identities"], other["columns"]) != (ref["identities"], ref["columns"])
        if cache is not None:
            cache[key] = out[:, t].copy()
    return out[0], out[1], out[2], changed


def pid_array(ident, cols, lens, pairs, denom):
    return np.array([python_pid(int(a), int(c), lens[i], lens[j], denom) for a, c, (i, j) in zip(ident, cols, pairs)], np.int64).astype(np.int32)


def device_identity(ctx, start, count, denom=COLUMNS, want=OUTPUTS, stream=0):
    """the outputs asked for, each in a poisoned tensor with 64 elements of room behind it"""
    import torch
    bufs = {name: torch.full((count + 64,), POISON, dtype=torch.int32, device="cuda") for name in want}
    torch.cuda.synchronize()
    ctx.identity_range(start, count, denom=denom, stream=stream, **{name: b.data_ptr() for name, b in bufs.items()})
    torch.cuda.synchronize()
    got = {}
    for name, b in bufs.items():
        host = b.cpu().numpy()
        assert (host[count:] == POISON).all(), f"sa_ctx_identity_range wrote beyond the range in {name}"
        got[name] = host[:count].copy()
    return got


def mismatch(name, got, want, pairs, lens):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    i, j = pairs[bad[0]]
    return f"{name}: {bad.size} of {len(want)} differ, first: pair {bad[0]} = ({i}, {j}), {lens[i]} x {lens[j]} residues: got {got[bad[0]]}, want {want[bad[0]]}"


def check_all(what, got, score, ident, cols, lens, pairs, denom):
    for name, want in (("score", score), ("identities", ident), ("columns", cols), ("pid", pid_array(ident, cols, lens, pairs, denom))):
        if name in got:
            bad = mismatch(name, got[name], want, pairs, lens)
            assert bad is None, f"{what}: {bad}"


# ---- 1. contract ---------------------------------------------------------------------------------------------------------------------
CONTRACT_CASES = [(m, x, g) for m, x, g in CONTRACT_SCORINGS] + [(m, "asym", tables.GAPS[m]) for m in tables.METHODS]


@pytest.mark.parametrize("method,matrix,gaps", CONTRACT_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_whole_triangle_equals_the_python_restatement(method, matrix, gaps, sa, oracle):
    seqs = make_protein_set(30, 1, 80, 11) + tie_heavy_sequences()
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = tables.scoring_with(sa, method, gaps, tables.asym(), lut=sa.Scoring.from_names(method, "blosum62", **gaps).lut) if matrix == "asym" \
        else sa.Scoring.from_names(method, matrix, **gaps)
    n = store.num
    pairs = packed_pairs(n)
    lens = [len(s) for s in seqs]
    assert n == 45 and len(pairs) == 990 == store.pairs and max(lens) == 80 > 64
    score, ident, cols, changed = reference(scoring, seqs, pairs, flipped=True)
    assert np.array_equal(score, oracle.align(store, scoring, triangular=True))  # the restatement's scores are the oracle's
    empty = int((cols == 0).sum())
    print(f"{method} {matrix} {gaps}: {changed} of 990 pairs change under the other tie order, {empty} empty alignments")
    if (method, matrix, gaps.get("gap_open"), gaps.get("gap_extend")) != ("sw", "blosum62", 10, 1):
        assert changed >= 30, "the case cannot tell the tie rule from another"  # 3 % of the pairs
    if scoring.method == 2:
        assert empty >= 1  # INT32_MIN under COLUMNS
    with sa.Context(store, scoring, 0) as ctx:
        for denom in DENOMS:
            got = device_identity(ctx, 0, len(pairs), denom)
            check_all(f"{method} {matrix} {gaps} denom {denom}", got, score, ident, cols, lens, pairs, denom)
        if empty:
            assert (got["pid"] >= 0).all() and (device_identity(ctx, 0, len(pairs), COLUMNS, ("pid",))["pid"] == INT32_MIN).sum() == empty
    # the one-call form: host triangles, any subset
    a, c, p = sa.hip_identity(store, scoring, denom=SHORTER)
    assert np.array_equal(a, ident) and np.array_equal(c, cols) and np.array_equal(p, pid_array(ident, cols, lens, pairs, SHORTER))
    assert sa.last_identity_seconds() > 0.0
    for k in range(0, len(pairs), 97):
        i, j = pairs[k]
        assert sa.pid_value(int(ident[k]), int(cols[k]), lens[i], lens[j], SHORTER) == int(p[k])


# ---- 2. strips ------------------------------------------------------------------------------------------------------------------------
STRIP_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]


@pytest.mark.parametrize("gaps", ["GAPS", "ZERO"])
@pytest.mark.parametrize("method", tables.METHODS)
def test_strip_edges(method, gaps, sa, oracle):
    seqs = tables.random_sequences(STRIP_LENGTHS, 23, "ARN")
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, "blosum62", **getattr(tables, gaps)[method])
    pairs = packed_pairs(store.num)
    score, ident, cols, _ = reference(scoring, seqs, pairs)
    assert np.array_equal(score, oracle.align(store, scoring, triangular=True))
    with sa.Context(store, scoring, 0) as ctx:
        got = device_identity(ctx, 0, len(pairs), MEAN)
        again = device_identity(ctx, 0, len(pairs), MEAN)
    check_all(f"{method} {gaps}", got, score, ident, cols, STRIP_LENGTHS, pairs, MEAN)
    assert all(np.array_equal(got[k], again[k]) for k in OUTPUTS)


# ---- 3. later trips -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", tables.METHODS)
def test_later_trips(method, sa, oracle):
    w = resident_waves()
    lengths = [1, 2, 63, 64, 65, 127, 128, 129, 140] + np.random.default_rng(31).integers(1, 141, 15).tolist()
    distinct = [make_protein_set(1, n, n, 3000 + k)[0] for k, n in enumerate(lengths)]
    assert len(distinct) == 24 and max(lengths) == 140
    rng = np.random.default_rng(32)
    pick = np.concatenate([np.arange(24), rng.integers(0, 24, 230 - 24)])
    rng.shuffle(pick)
    seqs = [distinct[k] for k in pick]
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
    pairs = packed_pairs(230)
    count = len(pairs)
    assert count == store.pairs and count > 2 * w, (count, w)
    lens = [len(s) for s in seqs]
    cells = np.array([lens[i] * lens[j] for i, j in pairs])
    assert (cells[w:2 * w] < cells[:w]).sum() > w // 4 and (cells[2 * w:3 * w] < cells[w:2 * w]).sum() > w // 4  # a shorter pair after a longer one
    cache = {}
    score, ident, cols, _ = reference(scoring, seqs, pairs, cache=cache)
    assert len(cache) <= 24 * 24
    assert np.array_equal(score, oracle.align(store, scoring, triangular=True, threads=16))
    with sa.Context(store, scoring, 0) as ctx:
        got = device_identity(ctx, 0, count, COLUMNS)
        again = device_identity(ctx, 0, count, COLUMNS)
    for name, want in (("score", score), ("identities", ident), ("columns", cols), ("pid", pid_array(ident, cols, lens, pairs, COLUMNS))):
        bad = np.flatnonzero(got[name] != want)
        assert bad.size == 0, (f"{method}: {bad.size} of {count} {name} differ, first: pair {bad[0]} = {pairs[bad[0]]} "
                               f"({lens[pairs[bad[0]][0]]} x {lens[pairs[bad[0]][1]]} residues, trip {bad[0] // w} of wave {bad[0] % w}, W = {w}): "
                               f"got {got[name][bad[0]]}, want {want[bad[0]]}")
        assert np.array_equal(again[name], got[name])


# ---- 4. ranges ------------------------------------------------------------------------------------------------------------------------
def test_ranges_subsets_and_in_place(sa, oracle):
    import torch
    seqs = make_protein_set(40, 5, 90, 41)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("ga", "blosum62", gap_open=10, gap_extend=1)
    pairs = packed_pairs(40)
    lens = [len(s) for s in seqs]
    score, ident, cols, _ = reference(scoring, seqs, pairs)
    assert np.array_equal(score, oracle.align(store, scoring, triangular=True))
    pid = pid_array(ident, cols, lens, pairs, LONGER)
    whole = dict(score=score, identities=ident, columns=cols, pid=pid)
    stream = torch.cuda.Stream()
    with sa.Context(store, scoring, 0) as ctx:
        # column 20 starts at 190, column 30 at 435: both ends mid-column; a range of one pair; the last pair; an empty range
        for start, count in ((197, 250), (3, 1), (779, 1), (0, 780), (400, 0)):
            got = device_identity(ctx, start, count, LONGER, stream=stream.cuda_stream)
            for name in OUTPUTS:
                assert np.array_equal(got[name], whole[name][start:start + count]), (name, start, count)
        for want in (("pid",), ("identities",), ("columns", "score"), ("score", "pid"), ("identities", "columns")):
            got = device_identity(ctx, 100, 333, LONGER, want)
            assert set(got) == set(want)
            for name in want:
                assert np.array_equal(got[name], whole[name][100:433]), want
        # pid in place over a buffer that holds the scores
        buf = torch.full((780 + 64,), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.align_range(0, 780, buf.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[:780], score)
        ctx.identity_range(0, 780, pid=buf.data_ptr(), denom=LONGER)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[:780], pid) and (host[780:] == POISON).all()
        # refusals: nothing written, and the context goes on working
        for kw, message in ((dict(start=0, count=781, pid=buf.data_ptr()), "outside the 780 pairs"), (dict(start=-1, count=1, pid=buf.data_ptr()), "outside"),
                            (dict(start=780, count=1, pid=buf.data_ptr()), "outside"), (dict(start=0, count=780), "every output is null"),
                            (dict(start=0, count=780, pid=buf.data_ptr(), denom=4), "denom 4 is none of"),
                            (dict(start=0, count=780, pid=buf.data_ptr(), denom=-1), "denom -1 is none of")):
            with pytest.raises(sa.AlignError, match=message):
                ctx.identity_range(**kw)
        ctx.identity_range(0, 780, identities=buf.data_ptr(), denom=99)  # denom is read iff pid
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[:780], ident)


def test_hip_identity_in_column_ranges(sa, monkeypatch):
    """the batch switch forcing many column-aligned ranges gives the bytes of one range"""
    store = sa.SequenceStore.from_sequences(make_protein_set(120, 10, 70, 43))
    scoring = sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1)
    monkeypatch.delenv("SA_HIP_IDENTITY_BATCH_BYTES", raising=False)
    one = sa.hip_identity(store, scoring, denom=COLUMNS)
    monkeypatch.setenv("SA_HIP_IDENTITY_BATCH_BYTES", str(3 * 4 * 700))  # 700 pairs: from one column up to six
    cut = sa.hip_identity(store, scoring, denom=COLUMNS)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, cut))
    only = sa.hip_identity(store, scoring, denom=None, identities=False)
    assert only[0] is None and only[2] is None and np.array_equal(only[1], one[1])


# ---- 5. device against device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", tables.METHODS)
def test_equals_the_records_of_the_device_traceback(method, sa):
    seqs = make_protein_set(300, 20, 120, 51)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, "blosum62", **tables.GAPS[method])
    pairs = np.array(packed_pairs(300), np.int32)
    assert len(pairs) == 44850
    with sa.Context(store, scoring, 0) as ctx:
        got = device_identity(ctx, 0, len(pairs), COLUMNS, ("score", "identities", "columns"))
        alns = ctx.alignments(pairs)
    for name in ("score", "identities", "columns"):
        bad = np.flatnonzero(got[name] != alns.records[name])
        assert bad.size == 0, f"{method}: {bad.size} {name} differ from sa_ctx_alignments, first: pair {pairs[bad[0]]}: {got[name][bad[0]]} / {alns.records[name][bad[0]]}"
    assert got["identities"].max() > 10 and (got["columns"] >= got["identities"]).all()


# ---- 6. selections, the tool, the tile job --------------------------------------------------------------------------------------------------
_sel = {}


def selection_case(sa, oracle):
    """60 proteins of 20 to 60 residues with planted near-duplicates, NW: store, scoring, the oracle's raw matrix, the pid
    triangle under COLUMNS from the Python restatement (computed once)"""
    if not _sel:
        seqs = make_near_duplicates(make_protein_set(60, 20, 60, 71), 0.4, 0.08, 71)
        store = sa.SequenceStore.from_sequences(seqs)
        scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
        pairs = packed_pairs(60)
        score, ident, cols, _ = reference(scoring, seqs, pairs)
        raw = oracle.align(store, scoring, triangular=True)
        assert np.array_equal(score, raw)
        pid = pid_array(ident, cols, [len(s) for s in seqs], pairs, COLUMNS)
        assert (pid >= 900000).sum() >= 5 and (pid < 900000).sum() > 1000  # near-duplicates above 90 %, the rest far below
        _sel["case"] = (seqs, store, scoring, tri_to_full(raw, 60), pid)
    return _sel["case"]


def test_selections_over_pid(sa, oracle):
    seqs, store, scoring, raw, pid = selection_case(sa, oracle)
    full = tri_to_full(pid, 60)
    tri = np.sort(pid)
    p = tri.size
    for k in (1, 5, 59):
        assert_same_neighbors(sa.hip_neighbors(store, scoring, k, pid=COLUMNS), expected_neighbors(full, k), f"k={k}")
    assert_same_edges(sa.hip_edges(store, scoring, 900000, pid=COLUMNS), expected_edges(full, 900000), "edges")
    assert_same_tree(sa.hip_linkage(store, scoring, pid=COLUMNS), prim_tree(full), "tree")
    ranks = [0, p - 1, p // 2, (95 * p) // 100]
    assert_same_select(sa.hip_select(store, scoring, ranks, pid=COLUMNS), expected_select(tri, ranks), "select")
    t = int(tri[ranks[3]])
    offsets, index, score, cut, under = sa.hip_edges_at_rank(store, scoring, ranks[3], pid=COLUMNS)
    assert cut == t and under == int(np.searchsorted(tri, t, "left"))
    assert_same_edges((offsets, index, score), expected_edges(full, t), "at rank")
    pairs, score, value, below = sa.hip_linkage_with_ranks(store, scoring, ranks, pid=COLUMNS)
    assert_same_tree((pairs, score), prim_tree(full), "with ranks")
    assert_same_select((value, below), expected_select(tri, ranks), "with ranks")
    assert sa.last_identity_seconds() > 0.0
    with pytest.raises(sa.AlignError, match="sa_hip_linkage_pid: denom 7 is none of"):
        sa.hip_linkage(store, scoring, pid=7)
    assert_same_neighbors(sa.hip_neighbors(store, scoring, 3), expected_neighbors(raw, 3), "the plain call after them: raw scores")


def test_tile_job_identity(sa, oracle):
    seqs, store, scoring, raw, pid = selection_case(sa, oracle)
    full = tri_to_full(pid, 60)
    tri = np.sort(pid)
    with sa.DeflateJob.begin(store, scoring, 64, level=1) as job:
        with pytest.raises(sa.AlignError, match="sa_zjob_identity: the walk is not finished"):
            job.identity(COLUMNS)
        while job.next():
            pass
        assert_same_neighbors(job.neighbors(5), expected_neighbors(raw, 5), "before identity: raw")
        with pytest.raises(sa.AlignError, match="denom 4 is none of"):
            job.identity(4)
        job.identity(COLUMNS)
        assert_same_neighbors(job.neighbors(5), expected_neighbors(full, 5), "tile job")
        assert_same_edges(job.edges(900000), expected_edges(full, 900000), "tile job")
        assert_same_tree(job.linkage(), prim_tree(full), "tile job")
        assert_same_select(job.select([0, tri.size - 1]), expected_select(tri, [0, tri.size - 1]), "tile job")
        with pytest.raises(sa.AlignError, match="percent identity already"):
            job.identity(COLUMNS)
        with pytest.raises(sa.AlignError, match="holds percent identity"):
            job.normalize(sa.Norm(sa.NORM_LENGTH, sa.NORM_MIN))
        assert_same_neighbors(job.neighbors(5), expected_neighbors(full, 5), "after the refusals")
    with sa.DeflateJob.begin(store, scoring, 64, level=1) as job:
        while job.next():
            pass
        job.normalize(sa.Norm(sa.NORM_LENGTH, sa.NORM_MIN))
        with pytest.raises(sa.AlignError, match="sa_zjob_identity: the job's matrix has been normalised already"):
            job.identity(COLUMNS)


def test_cli_identity(tmp_path, sa, oracle):
    from tests.host_binding import h5_matrix, h5_sequences
    from tests.test_edges_host import EDGE_SETS, h5_array, h5_edges
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_linkage_host import TREE_SETS, h5_linkage
    from tests.test_neighbors_host import h5_dataset, h5_names
    seqs, store, scoring, raw, pid = selection_case(sa, oracle)
    n = 60
    full = tri_to_full(pid, n)
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]
    out = tmp_path / "all.h5"
    res = run("-i", fasta, "-o", out, *flags, "-k", 5, "--min-score", 900000, "--clusters", 900000, "--identity", "columns", "-B", "-V")
    assert "Percent identity on the device, over columns" in res.stdout, res.stdout
    assert h5_names(out) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores", *EDGE_SETS, *TREE_SETS, "/cluster_labels",
                             "/identity_rule", "/identity_scale"}
    assert np.array_equal(h5_matrix(out, n), raw) and h5_sequences(out) == seqs  # the matrix stays raw
    assert_same_neighbors((h5_dataset(out, "neighbor_indices", (n, 5)), h5_dataset(out, "neighbor_scores", (n, 5))), expected_neighbors(full, 5), "tool")
    assert_same_edges(h5_edges(out, n), expected_edges(full, 900000), "tool")
    assert_same_tree(h5_linkage(out, n), prim_tree(full), "tool")
    assert np.array_equal(h5_array(out, "cluster_labels", "<i4"), labels_at(full, 900000)[0])
    assert h5_array(out, "identity_rule", "<i4").tolist() == [COLUMNS] and h5_array(out, "identity_scale", "<i4").tolist() == [SCALE]
    only = tmp_path / "only.h5"
    run("-i", fasta, "-o", only, *flags, "-k", 5, "--identity", "columns", "--neighbors-only", "-Q")
    assert h5_names(only) == {"/sequences", "/neighbor_indices", "/neighbor_scores", "/identity_rule", "/identity_scale"}
    assert_same_neighbors((h5_dataset(only, "neighbor_indices", (n, 5)), h5_dataset(only, "neighbor_scores", (n, 5))), expected_neighbors(full, 5),
                          "neighbors-only")

