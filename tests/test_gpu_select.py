"""GPU (-m gpu): exact order statistics of the score distribution selected on the device (sa_ctx_select / sa_hip_select /
sa_zjob_select / sa_hip_edges_at_rank / sa_hip_linkage_with_ranks, csrc/sa_select.hip; the tool's --min-quantile,
--clusters-quantile and --quantiles).  Contract (include/seqalign_hip.h): with the P = N (N - 1) / 2 pair scores in ascending
order, value = the score at rank k, below = the number of pairs that score strictly less.

The expected answer never comes from the code under test: it is np.sort(x)[rank] and np.searchsorted(np.sort(x), value, "left")
on a matrix from the oracle, on a synthetic tensor or, at config-2 size, on the packed matrix the reference-pinned alignment
delivers.  value and below are compared exactly, dtype and shape included."""
import subprocess

import numpy as np
import pytest

from tests.golden_util import tri_to_full
from tests.synth import make_dna_set, make_protein_set
from tests.test_gpu_edges import assert_same as assert_same_edges, expected_edges, packed_from
from tests.test_gpu_neighbors import oracle_case  # (the same stores and oracle matrices, computed once for all files)

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
POISON32, POISON64 = -0x5A5A5A5B, -0x5A5A5A5B5A5A5A5B


def expected_select(tri_sorted: np.ndarray, ranks):
    """the contract, with NumPy, from an ascending array"""
    value = tri_sorted[np.asarray(ranks, np.int64)].astype(np.int32)
    return value, np.searchsorted(tri_sorted, value, "left").astype(np.int64)


def assert_same(got, want, what=""):
    for name, g, w in zip(("value", "below"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} entries of {name} differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"


def python_rank(pairs, q):
    return min(pairs - 1, int(q * pairs))


# ---- 1. hip_select against the oracle: one element, three, fewer than a vector, many workgroups ---------------------------------
CASES = [(m, n) for n in (2, 3, 17, 65, 700) for m in ("nw", "ga", "sw")] + [("nw", 2100)]


@pytest.mark.parametrize("method,n", CASES)
def test_hip_select_equals_sort_of_the_oracle_matrix(method, n, sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, method, n)
    tri = np.sort(packed_from(full))
    p = tri.size
    assert p == n * (n - 1) // 2 and sa.score_rank(p, 0.99) == python_rank(p, 0.99)
    ranks = [0, p - 1, p // 2, sa.score_rank(p, 0.99), p // 2, 0]  # (two duplicates)
    shuffled = [ranks[k] for k in np.random.default_rng(n).permutation(len(ranks))]
    for r in (ranks, shuffled, [p // 2], [p - 1] * 16):
        assert_same(sa.hip_select(store, scoring, r), expected_select(tri, r), f"{method} N={n} ranks={r}")
    assert sa.last_select_seconds() > 0.0


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------
def test_below_counts_strictly_below_among_thousands_of_ties(sa, oracle):
    """short DNA under SW / nuc44 (the store of test_gpu_edges.test_entries_equal_to_the_threshold): few distinct scores, the
    median occurs thousands of times; below is the same for the first and the last rank that hold it"""
    store = sa.SequenceStore.from_sequences(make_dna_set(300, 120, 180, 4))
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    tri = np.sort(oracle.align(store, scoring, triangular=True))
    p = tri.size
    median = tri[p // 2]
    first, last = int(np.searchsorted(tri, median, "left")), int(np.searchsorted(tri, median, "right")) - 1
    print(f"median {median} occurs {last - first + 1} times among {p} pairs (ranks {first} .. {last})")
    assert last - first + 1 >= 1000
    ranks = [first, last, p // 2, max(first - 1, 0), min(last + 1, p - 1)]
    value, below = sa.hip_select(store, scoring, ranks)
    assert_same((value, below), expected_select(tri, ranks), "ties")
    assert value[:3].tolist() == [median] * 3 and below[:3].tolist() == [first] * 3
    if first > 0:
        assert value[3] < median and below[3] < first
    if last < p - 1:
        assert value[4] > median and below[4] == last + 1


# ---- 3. device-resident, synthetic contents: all four rounds, many groups -------------------------------------------------------
def synthetic(kind: str, p: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.integers(INT32_MIN, INT32_MAX, p, dtype=np.int64, endpoint=True).astype(np.int32)
        if p >= 3:
            x[rng.integers(0, p)] = INT32_MIN
            x[(np.flatnonzero(x != INT32_MIN))[0]] = INT32_MAX
        return x
    if kind == "equal":
        return np.full(p, -123456, np.int32)
    if kind == "pm":
        return rng.integers(-1, 0, p, endpoint=True).astype(np.int32)
    if kind == "extremes":
        return np.where(rng.integers(0, 2, p) == 1, INT32_MAX, INT32_MIN).astype(np.int32)
    assert kind == "band"
    return (70000 + rng.integers(0, 300, p)).astype(np.int32)


@pytest.mark.parametrize("n", [2, 23, 91, 700])
def test_context_select_on_a_stream_with_synthetic_contents(n, sa):
    import torch
    store = sa.SequenceStore.from_sequences(make_protein_set(n, 3, 5, 11))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    p = store.pairs
    rank_sets = ([k * p // 16 for k in range(16)], [p // 3] * 16)
    stream = torch.cuda.Stream()
    with sa.Context(store, scoring, 0) as ctx:
        for kind in ("uniform", "equal", "pm", "extremes", "band"):
            x = synthetic(kind, p, 100 * n + len(kind))
            tri = np.sort(x)
            if kind == "uniform" and p >= 4096:
                assert len({int(v) >> 24 for v in tri[rank_sets[0]]}) == 16  # sixteen ranks in sixteen top bytes: sixteen groups
            d_aligned = torch.from_numpy(x).cuda()
            d_longer = torch.cat([torch.full((1,), 99, dtype=torch.int32), torch.from_numpy(x)]).cuda()
            d_offset = d_longer[1:]  # 4-byte aligned only
            assert d_aligned.data_ptr() % 16 == 0 and d_offset.data_ptr() % 16 == 4
            for ranks in rank_sets:
                m = len(ranks)
                want = expected_select(tri, ranks)
                for d_packed in (d_aligned, d_offset):
                    d_value = torch.full((m + 1,), POISON32, dtype=torch.int32, device="cuda")
                    d_below = torch.full((m + 1,), POISON64, dtype=torch.int64, device="cuda")
                    d_scratch = torch.full((sa.select_scratch_bytes(m),), 0xFF, dtype=torch.uint8, device="cuda")
                    assert d_scratch.data_ptr() % 8 == 0
                    torch.cuda.synchronize()
                    ctx.select(d_packed.data_ptr(), ranks, d_value.data_ptr(), d_below.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
                    stream.synchronize()
                    value, below = d_value.cpu().numpy(), d_below.cpu().numpy()
                    assert value[m] == POISON32 and below[m] == POISON64, "written beyond m elements"
                    assert_same((value[:m], below[:m]), want, f"N={n} {kind} ranks={ranks[:3]}...")
            assert np.array_equal(d_aligned.cpu().numpy(), x) and d_longer[0].item() == 99  # (the input is read only)


# ---- 4. composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,n", [("nw", 700), ("sw", 65), ("ga", 2)])
def test_edges_at_rank_is_select_then_edges(method, n, sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, method, n)
    tri = np.sort(packed_from(full))
    p = tri.size
    for r in sorted({python_rank(p, 0.99), p // 2, 0, p - 1}):
        offsets, index, score, t, below = sa.hip_edges_at_rank(store, scoring, r)
        assert t == int(tri[r]) and below == int(np.searchsorted(tri, tri[r], "left"))
        assert_same_edges((offsets, index, score), expected_edges(full, t), f"{method} N={n} rank {r}")
        assert int(offsets[-1]) == 2 * (p - below)


def test_linkage_with_ranks_is_linkage_and_select(sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, "ga", 700)
    tri = np.sort(packed_from(full))
    ranks = [python_rank(tri.size, q) for q in (0.9, 0.0, 1.0, 0.5)]
    pairs, score, value, below = sa.hip_linkage_with_ranks(store, scoring, ranks)
    want_pairs, want_score = sa.hip_linkage(store, scoring)
    assert pairs.dtype == want_pairs.dtype and np.array_equal(pairs, want_pairs) and np.array_equal(score, want_score)
    assert_same((value, below), expected_select(tri, ranks), "with the tree")
    assert_same((value, below), sa.hip_select(store, scoring, ranks), "against hip_select")


def test_tile_job_select(sa, oracle, monkeypatch):
    n, chunk = 700, 256
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    tri = np.sort(packed_from(full))
    ranks = [python_rank(tri.size, q) for q in (0.99, 0.5, 0.0, 1.0)]
    want = expected_select(tri, ranks)
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        with pytest.raises(sa.AlignError) as early:
            job.select(ranks)  # the walk has not ended: the matrix is not there yet
        with pytest.raises(sa.AlignError) as early_edges:
            job.edges(0)
        assert "not finished" in str(early.value)
        assert str(early.value).replace("sa_zjob_select", "sa_zjob_edges") == str(early_edges.value)  # the same wording
        while job.next():
            pass
        assert_same(job.select(ranks), want, "tile job")
        assert_same(job.select(ranks), sa.hip_select(store, scoring, ranks), "tile job against hip_select")
    monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="dealt over 3 jobs"):
            job.select(ranks)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_the_process_lives_on(sa, oracle):
    import torch
    n = 65
    store, scoring, full = oracle_case(sa, oracle, "sw", n)
    tri = np.sort(packed_from(full))
    p = tri.size
    d_packed = torch.from_numpy(packed_from(full)).cuda()
    d_value = torch.full((17,), POISON32, dtype=torch.int32, device="cuda")
    d_below = torch.full((17,), POISON64, dtype=torch.int64, device="cuda")
    d_scratch = torch.zeros(sa.select_scratch_bytes(16), dtype=torch.uint8, device="cuda")
    pk, v, b, s = d_packed.data_ptr(), d_value.data_ptr(), d_below.data_ptr(), d_scratch.data_ptr()
    one = sa.SequenceStore.from_sequences(make_protein_set(1, 20, 30, 5))
    with sa.Context(store, scoring, 0) as ctx:
        for ranks, message in (([-1], "outside"), ([p], "outside"), ([0, p], "outside"), ([], "ranks|null"), ([0] * 17, "17 ranks")):
            with pytest.raises(sa.AlignError, match=message):
                ctx.select(pk, ranks, v, b, s)
            with pytest.raises(sa.AlignError, match=message):
                sa.hip_select(store, scoring, ranks)
            torch.cuda.synchronize()
            assert (d_value.cpu().numpy() == POISON32).all() and (d_below.cpu().numpy() == POISON64).all()
            ctx.select(pk, [p // 2], v, b, s)  # after each one a valid call succeeds
            torch.cuda.synchronize()
            assert d_value[0].item() == int(tri[p // 2]) and d_below[0].item() == int(np.searchsorted(tri, tri[p // 2], "left"))
            d_value.fill_(POISON32)
            d_below.fill_(POISON64)
        for args in ((0, [0], v, b, s), (pk, [0], 0, b, s), (pk, [0], v, 0, s), (pk, [0], v, b, 0)):
            with pytest.raises(sa.AlignError, match="null"):
                ctx.select(*args)
        torch.cuda.synchronize()
        assert (d_value.cpu().numpy() == POISON32).all() and (d_below.cpu().numpy() == POISON64).all()
        ctx.select(pk, [0, p - 1], v, b, s)
        torch.cuda.synchronize()
        assert d_value[:2].tolist() == [int(tri[0]), int(tri[-1])]
    with pytest.raises(sa.AlignError, match="no pair"):  # (a context over one sequence cannot be created: the host-to-host call refuses)
        sa.hip_select(one, scoring, [0])
    for rank in (-1, p):
        with pytest.raises(sa.AlignError, match="outside"):
            sa.hip_edges_at_rank(store, scoring, rank)
        with pytest.raises(sa.AlignError, match="outside"):
            sa.hip_linkage_with_ranks(store, scoring, [0, rank])
    assert_same(sa.hip_select(store, scoring, [0, p - 1]), expected_select(tri, [0, p - 1]), "a valid call after the errors")


# ---- 6. scale ---------------------------------------------------------------------------------------------------------------------
def test_config2_scale(sa):
    """10 000 proteins, 5 * 10^7 pairs: the grid stride over many vectors per thread and 64-bit counts that small N cannot show.
    The expectation comes from the GPU's own packed matrix copied to the host (pinned to the reference by test_gpu_digests.py)
    and np.partition; the selection is the only code under test."""
    import torch
    from tests.synth import make_config
    seqs, cfg = make_config("cfg2")
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    p = store.pairs
    ranks = [sa.score_rank(p, q) for q in (0, 0.5, 0.99, 0.999, 1)]
    assert ranks == [python_rank(p, q) for q in (0, 0.5, 0.99, 0.999, 1)] and ranks[0] == 0 and ranks[-1] == p - 1
    m = len(ranks)
    d_packed = torch.empty(p, dtype=torch.int32, device="cuda")
    d_value = torch.empty(m, dtype=torch.int32, device="cuda")
    d_below = torch.empty(m, dtype=torch.int64, device="cuda")
    d_scratch = torch.empty(sa.select_scratch_bytes(m), dtype=torch.uint8, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:
        ctx.align_range(0, p, d_packed.data_ptr())
        ctx.select(d_packed.data_ptr(), ranks, d_value.data_ptr(), d_below.data_ptr(), d_scratch.data_ptr())
        torch.cuda.synchronize()
    tri = d_packed.cpu().numpy()
    want_value = np.partition(tri, ranks)[ranks].astype(np.int32)
    want_below = np.array([int((tri < t).sum()) for t in want_value], np.int64)
    print(f"config 2: P = {p}, ranks {ranks}: values {want_value.tolist()}, below {want_below.tolist()}")
    assert_same((d_value.cpu().numpy(), d_below.cpu().numpy()), (want_value, want_below), "config 2")


# ---- 7. the tool ------------------------------------------------------------------------------------------------------------------
def test_cli_quantiles(tmp_path, sa, oracle):
    from tests.host_binding import H5DIFF, h5_sequences
    from tests.test_edges_host import EDGE_SETS, h5_array, h5_edges
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_neighbors_host import h5_names
    from tests.test_select_host import QUANTILE_SETS
    n = 300
    seqs = make_protein_set(n, 30, 80, 23)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    tri = oracle.align(store, scoring, triangular=True)
    full = tri_to_full(tri, n)
    tri = np.sort(tri)
    p = tri.size
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]

    def quantile_sets(path, fractions):
        ranks = [python_rank(p, q) for q in fractions]
        assert h5_array(path, "score_quantiles", "<f8").tolist() == fractions
        assert_same((h5_array(path, "score_quantile_values", "<i4"), h5_array(path, "score_quantile_below", "<i8")),
                    expected_select(tri, ranks), str(path))

    # --min-quantile: the score graph at the oracle's T, beside the matrix and instead of it
    t = int(tri[python_rank(p, 0.99)])
    want = expected_edges(full, t)
    plain, only = tmp_path / "minq.h5", tmp_path / "minq_only.h5"
    res = run("-i", fasta, "-o", plain, *flags, "--min-quantile", 0.99, "-B", "-V")
    assert f"Score graph: T = {t}, the score at rank {python_rank(p, 0.99)} of {p}" in res.stdout and "Score quantiles" in res.stdout, res.stdout
    assert h5_names(plain) == {"/sequences", "/similarity_matrix", *EDGE_SETS, *QUANTILE_SETS, "/edge_min_score"}
    res = run("-i", fasta, "-o", only, *flags, "--min-quantile=0.99", "--edges-only", "-B")
    assert "only the edges come back" in res.stdout, res.stdout
    assert h5_names(only) == {"/sequences", *EDGE_SETS, *QUANTILE_SETS, "/edge_min_score"}
    for path in (plain, only):
        assert_same_edges(h5_edges(path, n), want, str(path))
        assert h5_array(path, "edge_min_score", "<i4").tolist() == [t]
        quantile_sets(path, [0.99])
        assert h5_sequences(path) == seqs

    # --clusters-quantile: the labels of the tree at the oracle's T
    t = int(tri[python_rank(p, 0.9)])
    tree = sa.hip_linkage(store, scoring)
    labels, _ = sa.linkage_labels(*tree, n, t)
    beside, alone = tmp_path / "clq.h5", tmp_path / "clq_only.h5"
    run("-i", fasta, "-o", beside, *flags, "--linkage", "--clusters-quantile", 0.9, "-Q")
    run("-i", fasta, "-o", alone, *flags, "--linkage-only", "--clusters-quantile", 0.9, "-Q")
    assert "/similarity_matrix" in h5_names(beside) and "/similarity_matrix" not in h5_names(alone)
    for path in (beside, alone):
        assert np.array_equal(h5_array(path, "cluster_labels", "<i4"), labels), path
        assert h5_array(path, "cluster_min_score", "<i4").tolist() == [t]
        quantile_sets(path, [0.9])
    # (the labels themselves, from the oracle's matrix alone: the components of full >= t)
    from tests.linkage_ref import labels_at
    assert np.array_equal(labels, labels_at(full, t)[0])

    # --quantiles alone: three datasets, and the matrix as without the option
    without, with_q = tmp_path / "without.h5", tmp_path / "with_q.h5"
    run("-i", fasta, "-o", without, *flags, "-Q")
    run("-i", fasta, "-o", with_q, *flags, "--quantiles", "0,0.5,1", "-Q")
    assert h5_names(with_q) == {"/sequences", "/similarity_matrix", *QUANTILE_SETS}
    quantile_sets(with_q, [0.0, 0.5, 1.0])
    for dataset in ("/similarity_matrix", "/sequences"):
        diff = subprocess.run([str(H5DIFF), str(without), str(with_q), dataset], capture_output=True, text=True)
        assert diff.returncode == 0, diff.stdout + diff.stderr
    # the path that keeps no device matrix: a select of its own after the normal flow
    hostm = tmp_path / "hostm.h5"
    res = run("-i", fasta, "-o", hostm, *flags, "--quantiles", "0,0.5,1", "--min-quantile", 0.5, "-B", "-V", env={"SA_HOST_MATRIX": "1"})
    assert "second alignment pass" in res.stdout, res.stdout
    quantile_sets(hostm, [0.0, 0.5, 1.0, 0.5])
    assert_same_edges(h5_edges(hostm, n), expected_edges(full, int(tri[p // 2])), "host matrix")
