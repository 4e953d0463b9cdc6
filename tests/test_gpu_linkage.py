"""GPU (-m gpu): the single-linkage tree built on the device (sa_ctx_linkage / sa_hip_linkage / sa_zjob_linkage,
csrc/sa_linkage.hip) and its host-only readers (sa_linkage_labels, sa_linkage_merges).  Contract (include/seqalign_hip.h): the
maximum spanning tree of the score matrix under the total order (score descending, then packed index ascending), its N - 1
pairs sorted by that order.

The expected answer is always tests/linkage_ref.py on a matrix that does not come from the code under test.  Everything is
compared exactly: dtype, shape, every element."""
import math

import numpy as np
import pytest

from tests.golden_util import tri_to_full
from tests.linkage_ref import labels_at, labels_from_csr, packed_from, prim_tree
from tests.synth import make_dna_set
from tests.test_gpu_neighbors import oracle_case  # (the same stores and oracle matrices, computed once for all three files)

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def assert_same(got, want, what=""):
    for name, g, w in zip(("pairs", "score"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} entries of {name} differ, first at {bad[0]}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


def star(n, value):
    return (np.array([[0, j] for j in range(1, n)], np.int32).reshape(n - 1, 2), np.full(n - 1, value, np.int32))


# ---- 1. hip_linkage against the reference on the oracle's matrix: the edges of a 16-row and a 64-column block, many blocks ---
CASES = [(m, n) for n in (2, 3, 16, 17, 64, 65, 700) for m in ("nw", "ga", "sw")] + [("nw", 2100)]


@pytest.mark.parametrize("method,n", CASES)
def test_hip_linkage_equals_prim_on_the_oracle_matrix(method, n, sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, method, n)
    want = prim_tree(full)
    got = sa.hip_linkage(store, scoring)
    rounds = sa.last_linkage_rounds()
    print(f"{method} N={n}: {rounds} rounds, {sa.last_linkage_seconds() * 1e3:.3f} ms")
    assert_same(got, want, f"{method} N={n}")
    assert 1 <= rounds <= math.ceil(math.log2(n))
    tri = np.sort(packed_from(full))
    for t in (int(tri[tri.size // 2]), int(tri[int(0.99 * tri.size)]), int(tri[0]), int(tri[-1]), int(tri[-1]) + 1):
        want_labels, want_clusters = labels_at(full, t)
        labels, clusters = sa.linkage_labels(got[0], got[1], n, t)
        assert labels.dtype == np.int32 and labels.shape == (n,) and clusters == want_clusters, f"T={t}"
        assert np.array_equal(labels, want_labels), f"T={t}"
        offsets, index, _ = sa.hip_edges(store, scoring, t)
        assert np.array_equal(labels, labels_from_csr(offsets, index)), f"T={t}: not the components of hip_edges"
        if t == int(tri[0]):
            assert clusters == 1 and not labels.any()
        if t == int(tri[-1]) + 1:
            assert clusters == n and np.array_equal(labels, np.arange(n))
    merges = sa.linkage_merges(got[0], n)
    assert merges.dtype == np.int32 and merges.shape == (n - 1, 3)
    assert (merges[:, 0] < merges[:, 1]).all() and merges[-1, 2] == n and (merges[:, 1] < n + np.arange(n - 1)).all()


# ---- 2. ties -----------------------------------------------------------------------------------------------------------------
def test_heavily_tied_scores(sa, oracle):
    """short DNA under SW / nuc44: few distinct scores, so the tie rule decides most of the tree"""
    store = sa.SequenceStore.from_sequences(make_dna_set(300, 120, 180, 4))
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    full = tri_to_full(oracle.align(store, scoring, triangular=True), store.num)
    want = prim_tree(full)
    values, counts = np.unique(want[1], return_counts=True)
    repeated = int(counts[counts > 1].sum())
    print(f"{repeated} of the tree's {want[1].size} scores occur more than once in it ({values.size} distinct)")
    assert repeated >= want[1].size // 10  # (from the oracle's scores alone, before the device is asked)
    assert_same(sa.hip_linkage(store, scoring), want, "SW / nuc44, N = 300")


@pytest.mark.parametrize("n", [130, 66])
def test_all_sequences_identical(n, sa, oracle):
    seq = b"ARNDCQEGHILKMFPSTWYV" * 2
    store = sa.SequenceStore.from_sequences([seq] * n)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    common = int(oracle.align(sa.SequenceStore.from_sequences([seq] * 2), scoring, triangular=True)[0])
    assert_same(sa.hip_linkage(store, scoring), star(n, common), f"N={n}")
    assert sa.last_linkage_rounds() == 1


# ---- 3. synthetic matrices through a created job: no alignment involved --------------------------------------------------------
def job_tree(sa, full):
    import torch
    n = full.shape[0]
    d_packed = torch.from_numpy(packed_from(full)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, 256, d_packed_ptr=d_packed.data_ptr()) as job:
        got = job.linkage()
    assert np.array_equal(d_packed.cpu().numpy(), packed_from(full))  # (the input is read only)
    return got


def chain(n, scores):
    """every entry -1000 but score(i, i + 1) = scores[i]"""
    full = np.full((n, n), -1000, np.int32)
    i = np.arange(n - 1)
    full[i, i + 1] = full[i + 1, i] = scores
    return full


def test_ruler_takes_exactly_ten_rounds(sa):
    n = 1024
    i = np.arange(n - 1)
    ctz = np.array([((int(v) + 1) & -(int(v) + 1)).bit_length() - 1 for v in i])
    full = chain(n, 100 - ctz)
    assert_same(job_tree(sa, full), prim_tree(full), "ruler")
    assert sa.last_linkage_rounds() == 10


def test_ramp_hooks_one_chain_of_700(sa):
    n = 700
    full = chain(n, np.arange(n - 1))
    want = prim_tree(full)
    assert sorted(map(tuple, want[0].tolist())) == [(i, i + 1) for i in range(n - 1)]
    assert_same(job_tree(sa, full), want, "ramp")
    assert sa.last_linkage_rounds() == 1  # (one round: the relabel walks a chain of depth N - 2)


@pytest.mark.parametrize("value", [INT32_MIN, INT32_MAX])
def test_extreme_scores_are_scores(value, sa):
    """no candidate is not a score value: a matrix of nothing but INT32_MIN (or INT32_MAX) still gives the star"""
    n = 130
    full = np.full((n, n), value, np.int32)
    assert_same(job_tree(sa, full), star(n, value), f"all {value}")


def test_random_matrix_over_four_edge_values(sa):
    n = 65
    rng = np.random.default_rng(11)
    m = np.triu(rng.choice(np.array([INT32_MIN, -1, 0, INT32_MAX], np.int32), size=(n, n)), 1)
    full = (m + m.T).astype(np.int32)
    assert_same(job_tree(sa, full), prim_tree(full), "four values")


def test_jobs_that_cannot_answer_refuse(sa, oracle, monkeypatch):
    import torch
    n, chunk = 700, 256
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    want = prim_tree(full)
    d_full = torch.from_numpy(np.ascontiguousarray(full)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, chunk, d_full_ptr=d_full.data_ptr()) as job:
        with pytest.raises(sa.AlignError, match="packed"):
            job.linkage()
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        with pytest.raises(sa.AlignError, match="not finished"):
            job.linkage()
        while job.next():
            pass
        assert_same(job.linkage(), want, "tile job")
    monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="dealt over 3 jobs"):
            job.linkage()


# ---- 4. device-resident ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [700, 65])
def test_context_linkage_on_a_stream_writes_nothing_else(n, sa, oracle):
    import torch
    store, scoring, full = oracle_case(sa, oracle, "ga", n)
    want = prim_tree(full)
    poison, tail = -0x5A5A5A5B, 4096
    nbytes = sa.linkage_scratch_bytes(n)
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
            ctx.linkage(d_packed.data_ptr(), d_pairs.data_ptr(), d_score.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            pairs, score, scratch = d_pairs.cpu().numpy(), d_score.cpu().numpy(), d_scratch.cpu().numpy()
            assert (pairs[2 * (n - 1):] == poison).all(), "pairs written beyond 2 (N - 1) elements"
            assert (score[n - 1:] == poison).all(), "score written beyond N - 1 elements"
            assert (scratch[nbytes // 4:] == poison).all(), "scratch written beyond linkage_scratch_bytes(N)"
            results.append((pairs[:2 * (n - 1)].reshape(n - 1, 2), score[:n - 1]))
    assert_same(results[0], want, f"device-resident N={n}")
    assert_same(results[1], want, f"device-resident N={n}, dirty scratch")
    assert np.array_equal(tri_to_full(d_packed.cpu().numpy(), n), full)  # (the input is read only)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
def test_null_pointers_raise_and_the_process_lives_on(sa, oracle):
    import torch
    n = 65
    store, scoring, full = oracle_case(sa, oracle, "sw", n)
    d_packed = torch.zeros(store.pairs, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    d_scratch = torch.zeros(sa.linkage_scratch_bytes(n) // 4, dtype=torch.int32, device="cuda")
    p, o, s, w = d_packed.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 8 * n, d_scratch.data_ptr()
    with sa.Context(store, scoring, 0) as ctx:
        for args in ((0, o, s, w), (p, 0, s, w), (p, o, 0, w), (p, o, s, 0)):
            with pytest.raises(sa.AlignError, match="null"):
                ctx.linkage(*args)
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any() and not d_scratch.cpu().numpy().any()
    assert_same(sa.hip_linkage(store, scoring), prim_tree(full), "a valid call after the errors")


# ---- 6. scale ----------------------------------------------------------------------------------------------------------------
_config2 = {}


def config2(sa):
    """config 2 aligned device-resident; the packed matrix on the host (pinned to the reference by test_gpu_digests.py), the
    device's tree of it and of its 2 000-sequence prefix"""
    if not _config2:
        import torch
        from tests.synth import make_config
        seqs, cfg = make_config("cfg2")
        store = sa.SequenceStore.from_sequences(seqs)
        scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
        n, m = store.num, 2000
        d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
        d_pairs = torch.empty(2 * (n - 1), dtype=torch.int32, device="cuda")
        d_score = torch.empty(n - 1, dtype=torch.int32, device="cuda")
        d_scratch = torch.empty(sa.linkage_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        with sa.Context(store, scoring, 0) as ctx:
            ctx.align_range(0, store.pairs, d_packed.data_ptr())
            ctx.linkage(d_packed.data_ptr(), d_pairs.data_ptr(), d_score.data_ptr(), d_scratch.data_ptr())
            torch.cuda.synchronize()
        with sa.DeflateJob(n, 256, d_packed_ptr=d_packed.data_ptr()) as job:  # (the host-to-host call tells the rounds)
            again = job.linkage()
            rounds = sa.last_linkage_rounds()
        with sa.DeflateJob(m, 256, d_packed_ptr=d_packed.data_ptr()) as job:  # (the prefix's pairs are the first m (m - 1) / 2)
            prefix = job.linkage()
        _config2.update(n=n, m=m, tri=d_packed.cpu().numpy(), tree=(d_pairs.cpu().numpy().reshape(n - 1, 2), d_score.cpu().numpy()),
                        again=again, rounds=rounds, prefix=prefix)
    return _config2


def test_config2_scale(sa):
    """10 000 proteins: cross-block and 32-bit indexing errors that small N cannot show"""
    c = config2(sa)
    n, tri = c["n"], c["tri"]
    full = np.zeros((n, n), np.int32)
    for j in range(1, n):
        seg = tri[j * (j - 1) // 2: j * (j - 1) // 2 + j]
        full[:j, j] = seg
        full[j, :j] = seg
    want = prim_tree(full)
    k = int(0.99 * tri.size)
    t = int(np.partition(tri, k)[k])
    labels, clusters = sa.linkage_labels(c["tree"][0], c["tree"][1], n, t)
    print(f"config 2: {c['rounds']} rounds; {clusters} clusters at T(0.99) = {t}")
    assert_same(c["tree"], want, "config 2")
    assert_same(c["again"], want, "config 2, from a created job")
    assert 1 <= c["rounds"] <= math.ceil(math.log2(n))
    assert clusters == n - int((want[1] >= t).sum())


def test_config2_prefix_against_scipy(sa):
    """an anchor that does not depend on the tie rule: scipy's single linkage of max - score"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    c = config2(sa)
    m = c["m"]
    full = tri_to_full(c["tri"][:m * (m - 1) // 2], m)
    pairs, score = c["prefix"]
    top = int(score.max())
    assert top == int(c["tri"][:m * (m - 1) // 2].max())
    dist = (top - full).astype(np.float64)
    np.fill_diagonal(dist, 0.0)
    z = hierarchy.linkage(squareform(dist, checks=False), "single")
    assert np.array_equal(np.sort(z[:, 2]), np.sort((top - score.astype(np.int64)).astype(np.float64)))
    heights = np.sort(z[:, 2])
    for h in (heights[m // 4], heights[m // 2], heights[(9 * m) // 10]):
        flat = hierarchy.fcluster(z, t=h, criterion="distance")
        labels, clusters = sa.linkage_labels(pairs, score, m, top - int(h))
        assert clusters == np.unique(flat).size
        # the same partition: each of our labels meets exactly one of scipy's ids and the other way round
        assert np.unique(np.stack([labels, flat], axis=1), axis=0).shape[0] == clusters


# ---- 7. the tool -------------------------------------------------------------------------------------------------------------
def test_cli_linkage(tmp_path, sa, oracle):
    import subprocess
    from tests.host_binding import H5DIFF, h5_matrix, h5_sequences
    from tests.synth import make_protein_set
    from tests.test_edges_host import EDGE_SETS, h5_array
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_gpu_edges import expected_edges
    from tests.test_gpu_neighbors import expected_neighbors
    from tests.test_linkage_host import REFUSED, TREE_SETS, h5_linkage
    from tests.test_neighbors_host import h5_dataset, h5_names
    n = 1100
    seqs = make_protein_set(n, 30, 80, 17)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    tri = oracle.align(store, scoring, triangular=True)
    full = tri_to_full(tri, n)
    want = sa.hip_linkage(store, scoring)  # (the library's answer ...
    assert_same(want, prim_tree(full), "library")  # ... which is the reference's)
    t = int(np.sort(tri)[int(0.99 * tri.size)])
    want_labels, want_clusters = labels_at(full, t)
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]
    report = f"single-linkage tree on the device: {n - 1} merges, "

    for name, extra, env in (("plain", [], None), ("z9", ["-z", 9], None), ("hostmatrix", [], {"SA_HOST_MATRIX": "1"})):
        without, with_l, with_e = tmp_path / f"{name}.h5", tmp_path / f"{name}_l.h5", tmp_path / f"{name}_e.h5"
        run("-i", fasta, "-o", without, *flags, *extra, "-Q", env=env)
        res = run("-i", fasta, "-o", with_l, *flags, *extra, "--linkage", "-B", "-V", env=env)
        assert report in res.stdout and " rounds, " in res.stdout, res.stdout
        # "second alignment pass" appears exactly where it does for edges
        edges = run("-i", fasta, "-o", with_e, *flags, *extra, "--min-score", t, "-B", "-V", env=env)
        second = "second alignment pass" in res.stdout
        assert second == ("second alignment pass" in edges.stdout) == (env is not None or sa.device_count() != 1), res.stdout
        assert h5_names(with_l) == {"/sequences", "/similarity_matrix", *TREE_SETS}
        assert_same(h5_linkage(with_l, n), want, name)
        assert np.array_equal(h5_matrix(with_l, n), full) and h5_sequences(with_l) == seqs
        for dataset in ("/similarity_matrix", "/sequences"):
            diff = subprocess.run([str(H5DIFF), str(without), str(with_l), dataset], capture_output=True, text=True)
            assert diff.returncode == 0, diff.stdout + diff.stderr

    clusters = tmp_path / "clusters.h5"
    res = run("-i", fasta, "-o", clusters, *flags, f"--clusters={t}", "-B", "-V")
    assert report in res.stdout and f"clusters at score >= {t}: {want_clusters})" in res.stdout, res.stdout
    assert f"Clusters: {want_clusters} at score >= {t}" in res.stdout, res.stdout
    assert h5_names(clusters) == {"/sequences", "/similarity_matrix", *TREE_SETS, "/cluster_labels"}
    assert_same(h5_linkage(clusters, n), want, "--clusters")
    labels = h5_array(clusters, "cluster_labels", "<i4")
    assert labels.shape == (n,) and np.array_equal(labels, want_labels)

    only = tmp_path / "only.h5"
    res = run("-i", fasta, "-o", only, *flags, "--linkage-only", "-B")
    assert "only the single-linkage tree comes back" in res.stdout and report in res.stdout, res.stdout
    assert h5_names(only) == {"/sequences", *TREE_SETS}
    assert_same(h5_linkage(only, n), want, "--linkage-only")
    assert h5_sequences(only) == seqs
    assert only.stat().st_size < (tmp_path / "plain.h5").stat().st_size // 10

    # -W: the tree is still built (for timing), nothing is written
    res = run("-i", fasta, "-W", *flags, "--linkage", "-B")
    assert report in res.stdout, res.stdout

    # all three products in one run
    both, k = tmp_path / "both.h5", 10
    run("-i", fasta, "-o", both, *flags, "--linkage", "-k", k, "--min-score", t, "-Q")
    assert h5_names(both) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores", *EDGE_SETS, *TREE_SETS}
    assert_same(h5_linkage(both, n), want, "--linkage with -k and --min-score")
    wi, ws = expected_neighbors(full, k)
    assert np.array_equal(h5_dataset(both, "neighbor_indices", (n, k)), wi) and np.array_equal(h5_dataset(both, "neighbor_scores", (n, k)), ws)
    we = expected_edges(full, t)
    assert np.array_equal(h5_array(both, "edge_offsets", "<i8"), we[0]) and np.array_equal(h5_array(both, "edge_indices", "<i4"), we[1])

    # the refused combinations
    for bad, message in REFUSED:
        refused = tmp_path / "refused.h5"
        res = run("-i", fasta, "-o", refused, *flags, *bad, check=False)
        assert res.returncode == 1 and message in res.stderr, res.stdout + res.stderr
        assert not refused.exists()
