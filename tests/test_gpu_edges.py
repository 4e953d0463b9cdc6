"""GPU (-m gpu): the score graph built on the device (sa_ctx_edge_offsets / sa_ctx_edge_fill / sa_hip_edges / sa_zjob_edges,
csrc/sa_edges.hip; the tool's --min-score and --edges-only).  Contract (include/seqalign_hip.h): entry (r, c), c != r, is an
edge iff score(r, c) >= min_score; the result is the symmetric adjacency as CSR -- offsets int64[N + 1], index int32[E] with
every row's columns ascending, score int32[E].

The expected answer is always computed by NumPy from a matrix that does not come from the code under test: the boolean
full >= T without its diagonal, its row sums, its row-major nonzero.  All three arrays are compared exactly, dtype and shape
included."""
import subprocess

import numpy as np
import pytest

from tests.golden_util import tri_to_full
from tests.synth import make_dna_set, make_protein_set
from tests.test_gpu_neighbors import oracle_case  # (the same stores and oracle matrices, computed once for both files)

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def expected_edges(full: np.ndarray, t: int):
    """the contract, with NumPy; row-major nonzero is ascending c per row"""
    a = full >= t
    np.fill_diagonal(a, False)
    offsets = np.concatenate([[0], np.cumsum(a.sum(1, dtype=np.int64))]).astype(np.int64)
    return offsets, np.nonzero(a)[1].astype(np.int32), full[a].astype(np.int32)


def assert_same(got, want, what=""):
    for name, g, w in zip(("offsets", "index", "score"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} entries of {name} differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"
    assert got[0][-1] % 2 == 0, f"{what}: E is odd"


def packed_from(full: np.ndarray) -> np.ndarray:
    n = full.shape[0]
    return np.concatenate([full[:j, j] for j in range(1, n)]).astype(np.int32) if n > 1 else np.zeros(0, np.int32)


# ---- 1. hip_edges against the oracle: the edges of a 16-row and a 64-column block, a partial last block, many blocks ------
CASES = [(m, n) for n in (2, 16, 17, 64, 65, 700) for m in ("nw", "ga", "sw")] + [("nw", 2100)]


@pytest.mark.parametrize("method,n", CASES)
def test_hip_edges_equals_numpy_on_the_oracle_matrix(method, n, sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, method, n)
    tri = np.sort(packed_from(full))
    size = tri.size
    median, q99, lo, hi = int(tri[size // 2]), int(tri[int(0.99 * size)]), int(tri[0]), int(tri[-1])
    # from the oracle's scores alone, before the device is asked: the case does test >= and empty rows.  (N = 2 has one
    # pair, which is its own 0.99 quantile: both rows have degree 1 there and no row can be empty.)
    assert (tri == q99).any()
    degree99 = np.diff(expected_edges(full, q99)[0])
    print(f"{method} N={n}: T(0.99) = {q99} occurs {int((tri == q99).sum())} times, {int((degree99 == 0).sum())} rows of degree 0; "
          f"median T = {median}: largest degree {int(np.diff(expected_edges(full, median)[0]).max())}")
    if n > 2:
        assert (degree99 == 0).any()
    for t in (median, q99, lo, hi, hi + 1, INT32_MIN, INT32_MAX):
        want = expected_edges(full, t)
        if t in (lo, INT32_MIN):
            assert want[0][-1] == n * (n - 1)
        if t == hi:
            assert want[0][-1] >= 2
        if t in (hi + 1, INT32_MAX):
            assert want[0][-1] == 0 and not want[0].any()
        assert_same(sa.hip_edges(store, scoring, t), want, f"{method} N={n} T={t}")


# ---- 2. the boundary value ---------------------------------------------------------------------------------------------------
def test_entries_equal_to_the_threshold(sa, oracle):
    """short DNA under SW / nuc44: few distinct scores, so the median occurs in every row and >= against > shows at once"""
    store = sa.SequenceStore.from_sequences(make_dna_set(300, 120, 180, 4))
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    tri = oracle.align(store, scoring, triangular=True)
    full = tri_to_full(tri, store.num)
    t = int(np.sort(tri)[tri.size // 2])
    at = full == t
    np.fill_diagonal(at, False)
    rows = int(at.any(1).sum())
    print(f"T = {t}: {int((tri == t).sum())} of {tri.size} pairs score exactly T, {rows} of {store.num} rows hold such an entry")
    assert rows >= store.num // 10
    assert_same(sa.hip_edges(store, scoring, t), expected_edges(full, t), f"T = {t}")
    assert_same(sa.hip_edges(store, scoring, t + 1), expected_edges(full, t + 1), f"T + 1 = {t + 1}")


# ---- 3. all equal -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, 66])
def test_all_scores_equal(n, sa, oracle):
    """every sequence identical: at the common score every row is 0 .. n - 1 without r, one above it nothing is left"""
    seq = b"ARNDCQEGHILKMFPSTWYV" * 2
    store = sa.SequenceStore.from_sequences([seq] * n)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    common = int(oracle.align(sa.SequenceStore.from_sequences([seq] * 2), scoring, triangular=True)[0])
    offsets, index, score = sa.hip_edges(store, scoring, common)
    assert offsets.dtype == np.int64 and index.dtype == np.int32 and score.dtype == np.int32
    assert offsets.tolist() == [r * (n - 1) for r in range(n + 1)]
    for r in range(n):
        assert index[offsets[r]:offsets[r + 1]].tolist() == [c for c in range(n) if c != r], r
    assert (score == common).all() and score.shape == (n * (n - 1),)
    offsets, index, score = sa.hip_edges(store, scoring, common + 1)
    assert offsets.shape == (n + 1,) and not offsets.any() and index.shape == (0,) and score.shape == (0,)
    assert index.dtype == np.int32 and score.dtype == np.int32


# ---- 4. device-resident -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [700, 65])
def test_context_edges_on_a_stream_write_nothing_else(n, sa, oracle):
    import torch
    store, scoring, full = oracle_case(sa, oracle, "ga", n)
    t = int(np.sort(packed_from(full))[store.pairs // 2])
    want = expected_edges(full, t)
    e = int(want[0][-1])
    poison, tail = -0x5A5A5A5B, 4096
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_offsets = torch.full((n + 1 + tail,), poison, dtype=torch.int64, device="cuda")
    d_index = torch.full((e + tail,), poison, dtype=torch.int32, device="cuda")
    d_score = torch.full((e + tail,), poison, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with sa.Context(store, scoring, 0) as ctx:
        ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=stream.cuda_stream)
        ctx.edge_offsets(d_packed.data_ptr(), t, d_offsets.data_ptr(), stream=stream.cuda_stream)
        ctx.edge_fill(d_packed.data_ptr(), t, d_offsets.data_ptr(), d_index.data_ptr(), d_score.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
    offsets, index, score = d_offsets.cpu().numpy(), d_index.cpu().numpy(), d_score.cpu().numpy()
    assert (offsets[n + 1:] == poison).all(), "offsets written beyond N + 1 elements"
    assert (index[e:] == poison).all() and (score[e:] == poison).all(), "written beyond E elements"
    assert_same((offsets[:n + 1], index[:e], score[:e]), want, f"device-resident N={n}")
    assert np.array_equal(tri_to_full(d_packed.cpu().numpy(), n), full)  # (the input is read only)


# ---- 5. tile jobs -----------------------------------------------------------------------------------------------------------
def test_tile_job_edges(sa, oracle, monkeypatch):
    n, chunk = 700, 256
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    tri = np.sort(packed_from(full))
    thresholds = (int(tri[int(0.99 * tri.size)]), int(tri[tri.size // 2]), int(tri[-1]) + 1)
    want = {t: sa.hip_edges(store, scoring, t) for t in thresholds}
    assert_same(want[thresholds[0]], expected_edges(full, thresholds[0]))
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        with pytest.raises(sa.AlignError, match="not finished"):
            job.edges(thresholds[0])  # the walk has not ended: the matrix is not there yet
        while job.next():
            pass
        for t in thresholds:
            assert_same(job.edges(t), want[t], f"tile job T={t}")
    # dealt over three jobs: none of them holds the whole matrix
    monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="dealt over 3 jobs"):
            job.edges(thresholds[0])


def test_created_job_edges(sa, oracle):
    """sa_zjob_create over a caller's device matrix: packed -> any time; full -> refused"""
    import torch
    n = 700
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    packed = packed_from(full)
    t = int(np.sort(packed)[int(0.9 * packed.size)])
    d_packed = torch.from_numpy(packed).cuda()
    d_full = torch.from_numpy(np.ascontiguousarray(full)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, 256, d_packed_ptr=d_packed.data_ptr()) as job:
        assert_same(job.edges(t), expected_edges(full, t))
    with sa.DeflateJob(n, 256, d_full_ptr=d_full.data_ptr()) as job:
        with pytest.raises(sa.AlignError, match="packed"):
            job.edges(t)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------
def test_null_pointers_raise_and_the_process_lives_on(sa, oracle):
    import torch
    n = 65
    store, scoring, full = oracle_case(sa, oracle, "sw", n)
    t = int(np.sort(packed_from(full))[store.pairs // 2])
    d_packed = torch.zeros(store.pairs, dtype=torch.int32, device="cuda")
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(2 * n * n, dtype=torch.int32, device="cuda")
    p, o, i, s = d_packed.data_ptr(), d_offsets.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 4 * n * n
    with sa.Context(store, scoring, 0) as ctx:
        for args in ((0, t, o), (p, t, 0)):
            with pytest.raises(sa.AlignError, match="null"):
                ctx.edge_offsets(*args)
        for args in ((0, t, o, i, s), (p, t, 0, i, s), (p, t, o, 0, s), (p, t, o, i, 0)):
            with pytest.raises(sa.AlignError, match="null"):
                ctx.edge_fill(*args)
        for bad in (2**31, -2**31 - 1):
            with pytest.raises(sa.AlignError, match="int32"):
                ctx.edge_offsets(p, bad, o)
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any() and not d_offsets.cpu().numpy().any()
    with pytest.raises(sa.AlignError, match="int32"):
        sa.hip_edges(store, scoring, 2**31)
    assert_same(sa.hip_edges(store, scoring, t), expected_edges(full, t), "a valid call after the errors")


# ---- 7. scale ---------------------------------------------------------------------------------------------------------------
def test_config2_scale(sa):
    """10 000 proteins, T = the 0.99 quantile: cross-block and 32-bit indexing errors that small N cannot show.  The expectation
    comes from the GPU's own packed matrix copied to the host (pinned to the reference by test_gpu_digests.py) and NumPy on the
    10 000 x 10 000 boolean; the selection is the only code under test."""
    import torch
    from tests.synth import make_config
    seqs, cfg = make_config("cfg2")
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    n = store.num
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:
        ctx.align_range(0, store.pairs, d_packed.data_ptr())
        torch.cuda.synchronize()
        tri = d_packed.cpu().numpy()
        k = int(0.99 * tri.size)
        t = int(np.partition(tri, k)[k])
        ctx.edge_offsets(d_packed.data_ptr(), t, d_offsets.data_ptr())
        torch.cuda.synchronize()
        e = int(d_offsets[n].item())
        d_index = torch.empty(max(e, 1), dtype=torch.int32, device="cuda")
        d_score = torch.empty(max(e, 1), dtype=torch.int32, device="cuda")
        ctx.edge_fill(d_packed.data_ptr(), t, d_offsets.data_ptr(), d_index.data_ptr(), d_score.data_ptr())
        torch.cuda.synchronize()
    full = np.zeros((n, n), np.int32)
    for j in range(1, n):
        seg = tri[j * (j - 1) // 2: j * (j - 1) // 2 + j]
        full[:j, j] = seg
        full[j, :j] = seg
    want = expected_edges(full, t)
    print(f"config 2: T = {t}, E = {e} ({100.0 * e / (n * (n - 1)):.2f} % of the entries), largest degree {int(np.diff(want[0]).max())}")
    assert e == want[0][-1]
    assert_same((d_offsets.cpu().numpy(), d_index.cpu().numpy()[:e], d_score.cpu().numpy()[:e]), want, "config 2")


# ---- 8. the tool ------------------------------------------------------------------------------------------------------------
def test_cli_edges(tmp_path, sa, oracle):
    from tests.host_binding import H5DIFF, h5_matrix, h5_sequences
    from tests.test_edges_host import EDGE_SETS, h5_edges
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_gpu_neighbors import expected_neighbors
    from tests.test_neighbors_host import h5_dataset, h5_names
    n = 1100
    seqs = make_protein_set(n, 30, 80, 17)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    tri = oracle.align(store, scoring, triangular=True)
    full = tri_to_full(tri, n)
    t = int(np.sort(tri)[int(0.99 * tri.size)])
    want = expected_edges(full, t)
    e = int(want[0][-1])
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]
    report = f"score graph on the device, min score = {t}: {e} edges"

    for name, extra, env in (("plain", [], None), ("z9", ["-z", 9], None), ("hostmatrix", [], {"SA_HOST_MATRIX": "1"})):
        without, with_t = tmp_path / f"{name}.h5", tmp_path / f"{name}_t.h5"
        run("-i", fasta, "-o", without, *flags, *extra, "-Q", env=env)
        res = run("-i", fasta, "-o", with_t, *flags, *extra, "--min-score", t, "-B", "-V", env=env)
        assert report in res.stdout, res.stdout
        second = "second alignment pass" in res.stdout
        # one device, the tile path: the finished job is asked, nothing is aligned twice; the host-matrix path says it did
        assert second == (env is not None or sa.device_count() != 1), res.stdout
        assert h5_names(with_t) == {"/sequences", "/similarity_matrix", *EDGE_SETS}
        assert_same(h5_edges(with_t, n), want, name)
        assert np.array_equal(h5_matrix(with_t, n), full) and h5_sequences(with_t) == seqs
        for dataset in ("/similarity_matrix", "/sequences"):
            diff = subprocess.run([str(H5DIFF), str(without), str(with_t), dataset], capture_output=True, text=True)
            assert diff.returncode == 0, diff.stdout + diff.stderr

    only = tmp_path / "only.h5"
    res = run("-i", fasta, "-o", only, *flags, f"--min-score={t}", "--edges-only", "-B")
    assert "only the edges come back" in res.stdout and report in res.stdout, res.stdout
    assert h5_names(only) == {"/sequences", *EDGE_SETS}
    assert_same(h5_edges(only, n), want, "--edges-only")
    assert h5_sequences(only) == seqs
    assert only.stat().st_size < (tmp_path / "plain.h5").stat().st_size // 10

    # -W: the selection still runs (for timing), nothing is written
    res = run("-i", fasta, "-W", *flags, "--min-score", t, "-B")
    assert report in res.stdout, res.stdout

    # both products in one run
    both, k = tmp_path / "both.h5", 10
    run("-i", fasta, "-o", both, *flags, "--min-score", t, "-k", k, "-Q")
    assert h5_names(both) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores", *EDGE_SETS}
    assert_same(h5_edges(both, n), want, "--min-score with -k")
    wi, ws = expected_neighbors(full, k)
    assert np.array_equal(h5_dataset(both, "neighbor_indices", (n, k)), wi) and np.array_equal(h5_dataset(both, "neighbor_scores", (n, k)), ws)
