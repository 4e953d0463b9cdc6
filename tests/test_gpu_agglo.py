"""GPU (-m gpu): complete and average linkage built on the device (sa_ctx_agglomerate / sa_hip_agglomerate* /
sa_zjob_agglomerate, csrc/sa_agglo.hip), the host-only sa_agglo_labels and the tool's --linkage-method.  Contract
(include/seqalign_hip.h): greedy agglomeration under the total order (similarity descending, then the packed index of the two
cluster names ascending); complete: minima; average: exact rationals, compared in 128 bits.

The expected answer is always tests/agglo_ref.py on a matrix that does not come from the code under test.  Everything is
compared exactly: dtype, shape, every element."""
import numpy as np
import pytest

from tests.agglo_ref import AVERAGE, COMPLETE, agglo_numpy, labels_of, merge_table, tie_free_full
from tests.golden_util import tri_to_full
from tests.linkage_ref import packed_from, random_full
from tests.test_gpu_neighbors import oracle_case  # (the same stores and oracle matrices as the neighbour / graph / tree files)

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
NAMES = {COMPLETE: "complete", AVERAGE: "average"}
BOTH = pytest.mark.parametrize("agglo", [COMPLETE, AVERAGE], ids=NAMES.get)


def assert_same(got, want, what=""):
    for name, g, w in zip(("pairs", "score"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} entries of {name} differ, first at {bad[0]}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


_expected = {}


def expected(key, full, agglo):
    """the reference's tree, computed once per matrix and method and left unchanged"""
    if (key, agglo) not in _expected:
        pairs, score = agglo_numpy(full, agglo)
        pairs.setflags(write=False)
        score.setflags(write=False)
        _expected[key, agglo] = (pairs, score)
    return _expected[key, agglo]


def inside_clusters_at_least(full, labels, t):
    same = labels[:, None] == labels[None, :]
    np.fill_diagonal(same, False)
    return bool((full[same] >= t).all())


# ---- 1. hip_agglomerate against the reference on the oracle's matrix; labels --------------------------------------------------
@BOTH
@pytest.mark.parametrize("n", [2, 3, 16, 17, 64, 65, 257, 700])
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_hip_agglomerate_equals_the_reference_on_the_oracle_matrix(method, n, agglo, sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, method, n)
    want = expected((method, n), full, agglo)
    got = sa.hip_agglomerate(store, scoring, NAMES[agglo])
    print(f"{method} N={n} {NAMES[agglo]}: {sa.last_agglomerate_seconds() * 1e3:.3f} ms, {sa.last_agglomerate_rescans()} rescans")
    assert_same(got, want, f"{method} N={n} {NAMES[agglo]}")
    assert 0 <= sa.last_agglomerate_rescans() <= (n - 1) * (n - 2)
    assert tuple(got[0][0]) == tuple(sa.hip_linkage(store, scoring)[0][0]), "the first merge is the first pair of the single-linkage tree"
    assert np.array_equal(sa.linkage_merges(got[0], n), merge_table(want[0], n))
    # labels at five thresholds, above the maximum and below the minimum among them
    score = want[1].astype(np.int64)
    for t in (int(score.max()) + 1, int(score.max()), int(np.median(score)), int(score.min()), int(score.min()) - 1):
        want_labels, want_clusters = labels_of(want[0], want[1], n, t)
        labels, clusters = sa.agglo_labels(got[0], got[1], n, t)
        assert labels.dtype == np.int32 and labels.shape == (n,) and clusters == want_clusters and np.array_equal(labels, want_labels), f"T={t}"
        if agglo == COMPLETE:
            assert inside_clusters_at_least(full, labels, t), f"T={t}: a pair inside a cluster of the ORIGINAL matrix scores below T"
    assert sa.agglo_labels(got[0], got[1], n, int(score.max()) + 1)[1] == n and sa.agglo_labels(got[0], got[1], n, int(score.min()))[1] == 1


# ---- 2. synthetic matrices through a created job: no alignment involved ---------------------------------------------------------
def job_tree(sa, full, agglo):
    import torch
    n = full.shape[0]
    d_packed = torch.from_numpy(packed_from(full)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, 256, d_packed_ptr=d_packed.data_ptr()) as job:
        got = job.agglomerate(agglo)
    assert np.array_equal(d_packed.cpu().numpy(), packed_from(full))  # (the input is read only)
    return got


@BOTH
@pytest.mark.parametrize("value", [INT32_MIN, INT32_MAX, 0])
def test_all_equal_is_the_star_without_a_rescan(value, agglo, sa):
    """no candidate is not a score value; and the keep-without-rescan rule: without it this costs N^3"""
    n = 257
    full = np.full((n, n), value, np.int32)
    pairs, score = job_tree(sa, full, agglo)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, t + 1] for t in range(n - 1)]
    assert score.dtype == np.int32 and (score == value).all()
    assert sa.last_agglomerate_rescans() == 0


@BOTH
def test_heavy_ties(agglo, sa):
    full = random_full(130, 3, 21)
    assert_same(job_tree(sa, full, agglo), agglo_numpy(full, agglo), "spread 3")


@BOTH
def test_star_invalidates_every_cache(agglo, sa):
    n = 257
    full = np.full((n, n), -100, np.int32)
    full[0, :] = full[:, 0] = 100
    assert_same(job_tree(sa, full, agglo), agglo_numpy(full, agglo), "star")
    assert sa.last_agglomerate_rescans() <= (n - 1) * (n - 2)


@BOTH
def test_random_matrix_over_four_edge_values(agglo, sa):
    n = 65
    rng = np.random.default_rng(11)
    m = np.triu(rng.choice(np.array([INT32_MIN, -1, 0, INT32_MAX], np.int32), size=(n, n)), 1)
    full = (m + m.T).astype(np.int32)
    assert_same(job_tree(sa, full, agglo), agglo_numpy(full, agglo), "four values")


@BOTH
def test_tie_free_matrix_against_scipy(agglo, sa):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    n = 300
    full = tie_free_full(n, 5)
    pairs, score = job_tree(sa, full, agglo)
    dist = -full.astype(np.float64)
    np.fill_diagonal(dist, 0.0)
    z = hierarchy.linkage(squareform(dist, checks=False), NAMES[agglo])
    table = sa.linkage_merges(pairs, n)
    assert np.array_equal(table[:, :2], z[:, :2].astype(np.int64)) and np.array_equal(table[:, 2], z[:, 3].astype(np.int64))
    assert np.array_equal(score, np.floor(-z[:, 2]).astype(np.int64))


def test_near_ties_of_averages_need_exact_arithmetic(sa):
    """entries 2^30 - r, r in 0 .. 3: sums near 2^30 n whose averages differ late in the mantissa or not at all.  The condition
    on the input is taken from the reference's exact run alone: some decision had a runner-up within 2^-53 relative of the winner
    (printed: the closest one).  At N = 130 two DIFFERENT averages are at least 1 / (n1 n2) > 2^-22.1 apart (n1 n2 <= 65^2 * 32 *
    33 < 2^23), more than 2^-53 of 2^30: what meets the condition here are exact ties -- among them, and asserted too, ties of
    the same rational in different terms (S, n), which only cross-multiplication sees as equal and the packed index decides."""
    from fractions import Fraction
    n = 130
    full = (2**30 - random_full(n, 4, 77).astype(np.int64) % 4).astype(np.int32)
    np.fill_diagonal(full, 0)
    stats = {}
    want = agglo_numpy(full, AVERAGE, stats)
    print(f"closest runner-up: {float(stats['closest']):.3e} relative; {stats.get('mixed_ties', 0)} decisions among equal averages in different terms")
    assert stats["closest"] <= Fraction(1, 2**53) and stats.get("mixed_ties", 0) >= 1
    assert_same(job_tree(sa, full, AVERAGE), want, "near ties")


# ---- 3. device-resident -----------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("n", [700, 65])
def test_context_agglomerate_on_a_stream_writes_nothing_else(n, agglo, sa, oracle):
    import torch
    store, scoring, full = oracle_case(sa, oracle, "ga", n)
    want = expected(("ga", n), full, agglo)
    poison, tail = -0x5A5A5A5B, 4096
    nbytes = sa.agglo_scratch_bytes(n, agglo)
    assert nbytes % 4 == 0 and nbytes > 0
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_scratch = torch.full((nbytes // 4 + tail,), poison, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    results = []
    with sa.Context(store, scoring, 0) as ctx:
        ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=stream.cuda_stream)
        for _ in range(2):  # the second call finds the scratch as the first one left it
            d_pairs = torch.full((2 * (n - 1) + tail,), poison, dtype=torch.int32, device="cuda")
            d_score = torch.full((n - 1 + tail,), poison, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.agglomerate(d_packed.data_ptr(), agglo, d_pairs.data_ptr(), d_score.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            pairs, score, scratch = d_pairs.cpu().numpy(), d_score.cpu().numpy(), d_scratch.cpu().numpy()
            assert (pairs[2 * (n - 1):] == poison).all(), "pairs written beyond 2 (N - 1) elements"
            assert (score[n - 1:] == poison).all(), "score written beyond N - 1 elements"
            assert (scratch[nbytes // 4:] == poison).all(), "scratch written beyond agglo_scratch_bytes(N, method)"
            results.append((pairs[:2 * (n - 1)].reshape(n - 1, 2), score[:n - 1]))
    assert_same(results[0], want, f"device-resident N={n}")
    assert_same(results[1], want, f"device-resident N={n}, dirty scratch")
    assert np.array_equal(tri_to_full(d_packed.cpu().numpy(), n), full)  # (the input is read only)


# ---- 4. quantities: the tree of normalised scores and of percent identity --------------------------------------------------------
@BOTH
def test_tree_of_normalised_scores(agglo, sa, oracle):
    import torch
    n = 64
    store, scoring, _ = oracle_case(sa, oracle, "nw", n)
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_den = torch.empty(n, dtype=torch.int32, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:  # (the existing calls give the normalised triangle: this anchors the plumbing)
        ctx.align_range(0, store.pairs, d_packed.data_ptr())
        ctx.denominators(sa.NORM_SELF, d_den.data_ptr())
        ctx.normalize(d_packed.data_ptr(), d_den.data_ptr(), sa.NORM_MIN, d_packed.data_ptr())
        torch.cuda.synchronize()
    normed = tri_to_full(d_packed.cpu().numpy(), n)
    pairs, score, den = sa.hip_agglomerate(store, scoring, agglo, norm=sa.Norm(sa.NORM_SELF, sa.NORM_MIN))
    assert_same((pairs, score), agglo_numpy(normed, agglo), "normalised")
    assert np.array_equal(den, d_den.cpu().numpy())


@BOTH
def test_tree_of_percent_identity(agglo, sa, oracle):
    n = 64
    store, scoring, _ = oracle_case(sa, oracle, "nw", n)
    pid = tri_to_full(sa.hip_identity(store, scoring, denom=sa.PID_COLUMNS)[2], n)
    assert_same(sa.hip_agglomerate(store, scoring, agglo, pid=sa.PID_COLUMNS), agglo_numpy(pid, agglo), "percent identity")


def test_with_ranks_is_the_tree_and_the_order_statistics(sa, oracle):
    n = 65
    store, scoring, full = oracle_case(sa, oracle, "sw", n)
    ranks = [0, store.pairs // 2, store.pairs - 1]
    pairs, score, values, below = sa.hip_agglomerate_with_ranks(store, scoring, "average", ranks)
    assert_same((pairs, score), expected(("sw", n), full, AVERAGE), "with ranks")
    tri = np.sort(packed_from(full))
    assert values.tolist() == [int(tri[r]) for r in ranks] and below.tolist() == [int((tri < tri[r]).sum()) for r in ranks]
    with pytest.raises(sa.AlignError, match="rank"):
        sa.hip_agglomerate_with_ranks(store, scoring, "average", [store.pairs])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_jobs_that_cannot_answer_refuse(sa, oracle, monkeypatch):
    import torch
    n, chunk = 700, 256
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    want = expected(("nw", n), full, COMPLETE)
    d_full = torch.from_numpy(np.ascontiguousarray(full)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, chunk, d_full_ptr=d_full.data_ptr()) as job:
        with pytest.raises(sa.AlignError, match="sa_zjob_agglomerate: the job walks a full matrix; the tree reads the packed index"):
            job.agglomerate("complete")
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        with pytest.raises(sa.AlignError, match="not finished"):
            job.agglomerate("complete")
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="method 0 is single linkage"):
            job.agglomerate(0)
        assert_same(job.agglomerate("complete"), want, "tile job")
    monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="dealt over 3 jobs"):
            job.agglomerate("average")


def test_null_pointers_and_method_0_raise_and_the_process_lives_on(sa, oracle):
    import torch
    n = 65
    store, scoring, full = oracle_case(sa, oracle, "sw", n)
    d_packed = torch.zeros(store.pairs, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    d_scratch = torch.zeros(sa.agglo_scratch_bytes(n, AVERAGE) // 4, dtype=torch.int32, device="cuda")
    p, o, s, w = d_packed.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 8 * n, d_scratch.data_ptr()
    with sa.Context(store, scoring, 0) as ctx:
        for args in ((0, 2, o, s, w), (p, 2, 0, s, w), (p, 2, o, 0, w), (p, 2, o, s, 0)):
            with pytest.raises(sa.AlignError, match="null"):
                ctx.agglomerate(*args)
        with pytest.raises(sa.AlignError, match="sa_ctx_linkage"):
            ctx.agglomerate(p, 0, o, s, w)
        with pytest.raises(sa.AlignError, match="method 3 is neither"):
            ctx.agglomerate(p, 3, o, s, w)
        with pytest.raises(sa.AlignError, match="not aligned"):
            ctx.agglomerate(p, 2, o, s, w + 4)
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any() and not d_scratch.cpu().numpy().any()
    assert_same(sa.hip_agglomerate(store, scoring, "average"), expected(("sw", n), full, AVERAGE), "a valid call after the errors")


# ---- 6. invariants at size ----------------------------------------------------------------------------------------------------------
@BOTH
def test_invariants_at_2100(agglo, sa, oracle):
    n = 2100
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    pairs, score = sa.hip_agglomerate(store, scoring, agglo)
    print(f"N={n} {NAMES[agglo]}: {sa.last_agglomerate_seconds() * 1e3:.1f} ms, {sa.last_agglomerate_rescans()} rescans")
    assert pairs.dtype == np.int32 and pairs.shape == (n - 1, 2) and score.dtype == np.int32 and score.shape == (n - 1,)
    assert (pairs[:, 0] < pairs[:, 1]).all() and pairs.min() >= 0 and pairs.max() < n
    assert (np.diff(score.astype(np.int64)) <= 0).all()
    merges = sa.linkage_merges(pairs, n)  # (refuses anything that is not a spanning tree)
    assert merges[-1, 2] == n
    assert np.unique(pairs[:, 1]).size == n - 1 and 0 not in pairs[:, 1]  # every name but 0 is merged away exactly once
    tri = packed_from(full)
    assert int(score[0]) == int(tri.max())
    if agglo == COMPLETE:
        assert int(score[-1]) == int(tri.min())  # (the last merge joins everything: its minimum is the matrix's)
        for t in (int(score[n // 4]), int(score[n // 2]), int(score[(9 * n) // 10])):
            labels, clusters = sa.agglo_labels(pairs, score, n, t)
            assert clusters == n - int((score >= t).sum())
            assert inside_clusters_at_least(full, labels, t), f"T={t}"


# ---- 7. the tool ----------------------------------------------------------------------------------------------------------------------
def test_cli_linkage_method(tmp_path, sa, oracle):
    from tests.host_binding import h5_sequences
    from tests.synth import make_protein_set
    from tests.test_edges_host import h5_array
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_linkage_host import TREE_SETS, h5_linkage
    from tests.test_neighbors_host import h5_names
    n = 300
    seqs = make_protein_set(n, 30, 80, 23)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    tri = oracle.align(store, scoring, triangular=True)
    full = tri_to_full(tri, n)
    complete, average = sa.hip_agglomerate(store, scoring, "complete"), sa.hip_agglomerate(store, scoring, "average")
    assert_same(complete, agglo_numpy(full, COMPLETE), "library, complete")  # (the library's answers are the reference's)
    assert_same(average, agglo_numpy(full, AVERAGE), "library, average")
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]

    def method_of(path):
        got = h5_array(path, "linkage_method", "<i4")
        assert got.shape == (1,)
        return int(got[0])

    # --linkage --linkage-method complete --clusters T
    t = int(np.sort(tri)[int(0.9 * tri.size)])
    want_labels, want_clusters = sa.agglo_labels(complete[0], complete[1], n, t)
    out = tmp_path / "complete.h5"
    res = run("-i", fasta, "-o", out, *flags, "--linkage", "--linkage-method", "complete", f"--clusters={t}", "-B", "-V")
    assert f"complete-linkage tree on the device: {n - 1} merges, " in res.stdout and f"Clusters: {want_clusters} at score >= {t}" in res.stdout, res.stdout
    assert h5_names(out) == {"/sequences", "/similarity_matrix", *TREE_SETS, "/cluster_labels", "/linkage_method"}
    assert_same(h5_linkage(out, n), complete, "--linkage-method complete")
    labels = h5_array(out, "cluster_labels", "<i4")
    assert np.array_equal(labels, want_labels) and inside_clusters_at_least(full, labels, t) and method_of(out) == 1

    # --linkage-only --linkage-method average
    only = tmp_path / "only.h5"
    res = run("-i", fasta, "-o", only, *flags, "--linkage-only", "--linkage-method", "average", "-B")
    assert "only the average-linkage tree comes back" in res.stdout and f"average-linkage tree on the device: {n - 1} merges, " in res.stdout, res.stdout
    assert h5_names(only) == {"/sequences", *TREE_SETS, "/linkage_method"} and h5_sequences(only) == seqs
    assert_same(h5_linkage(only, n), average, "--linkage-only --linkage-method average")
    assert method_of(only) == 2

    # -z 6: the tile-job path
    tiled = tmp_path / "z6.h5"
    run("-i", fasta, "-o", tiled, *flags, "-z", 6, "--linkage", "--linkage-method=average", "-Q")
    assert_same(h5_linkage(tiled, n), average, "-z 6")
    assert method_of(tiled) == 2

    # --clusters-quantile 0.9: the cut comes from the same device matrix
    quant = tmp_path / "quantile.h5"
    res = run("-i", fasta, "-o", quant, *flags, "--linkage-method", "complete", "--clusters-quantile", 0.9, "-B", "-V")
    tq = int(np.sort(tri)[sa.score_rank(tri.size, 0.9)])
    want_labels, want_clusters = sa.agglo_labels(complete[0], complete[1], n, tq)
    assert f"Clusters: {want_clusters} at score >= {tq}" in res.stdout, res.stdout
    assert_same(h5_linkage(quant, n), complete, "--clusters-quantile")
    assert np.array_equal(h5_array(quant, "cluster_labels", "<i4"), want_labels) and method_of(quant) == 1

    # --identity columns: the tree of percent identity
    ident = tmp_path / "identity.h5"
    run("-i", fasta, "-o", ident, *flags, "--identity", "columns", "--linkage-only", "--linkage-method", "complete", "-Q")
    assert_same(h5_linkage(ident, n), sa.hip_agglomerate(store, scoring, "complete", pid=sa.PID_COLUMNS), "--identity columns")
    assert method_of(ident) == 1

    # the option spelled out as single is single linkage, and says so; without it nothing is new
    single = tmp_path / "single.h5"
    run("-i", fasta, "-o", single, *flags, "--linkage-only", "--linkage-method", "single", "-Q")
    assert_same(h5_linkage(single, n), sa.hip_linkage(store, scoring), "--linkage-method single")
    assert method_of(single) == 0
    plain = tmp_path / "plain.h5"
    run("-i", fasta, "-o", plain, *flags, "--linkage", "-Q")
    assert h5_names(plain) == {"/sequences", "/similarity_matrix", *TREE_SETS}
    assert_same(h5_linkage(plain, n), sa.hip_linkage(store, scoring), "--linkage alone")
