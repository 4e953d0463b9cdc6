"""GPU (-m gpu): nearest neighbours selected on the device (sa_ctx_neighbors / sa_hip_neighbors / sa_zjob_neighbors,
csrc/sa_neighbors.hip; the tool's -k option).  Contract (include/seqalign_hip.h): row r lists the c != r by score
descending, then index ascending -- k of them, index and score.

The expected answer is always computed by NumPy from a matrix that does not come from the code under test:
np.lexsort((cols, -scores)) per row of the oracle's matrix.  Everything is compared exactly, both arrays."""
import subprocess
import time

import numpy as np
import pytest

from tests.golden_util import tri_to_full
from tests.synth import make_dna_set, make_protein_set

pytestmark = pytest.mark.gpu

GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}


def expected_neighbors(full: np.ndarray, k: int):
    """the contract, with NumPy: per row a lexsort by (score descending, column ascending) of every column but the row's own"""
    n = full.shape[0]
    index, score = np.empty((n, k), np.int32), np.empty((n, k), np.int32)
    every = np.arange(n)
    for r in range(n):
        cols = np.delete(every, r)
        scores = full[r, cols].astype(np.int64)
        order = np.lexsort((cols, -scores))[:k]
        index[r], score[r] = cols[order], scores[order]
    return index, score


def assert_same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == np.int32 and gs.dtype == np.int32 and gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.argwhere((gi != wi) | (gs != ws))
    assert bad.size == 0, (f"{what}: {len(bad)} entries differ, first at row {bad[0][0]} place {bad[0][1]}: "
                           f"got ({gi[tuple(bad[0])]}, {gs[tuple(bad[0])]}), want ({wi[tuple(bad[0])]}, {ws[tuple(bad[0])]})")


_cache = {}


def oracle_case(sa, oracle, method: str, n: int):
    """store, scoring and the oracle's full matrix of n short proteins (computed once per method and size)"""
    key = (method, n)
    if key not in _cache:
        store = sa.SequenceStore.from_sequences(make_protein_set(n, 20, 60, 30 + n))
        scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
        _cache[key] = (store, scoring, tri_to_full(oracle.align(store, scoring, triangular=True), n))
    return _cache[key]


def k_values(n):
    return sorted({1, min(7, n - 1), min(64, n - 1)})


# ---- 1. hip_neighbors against the oracle: row-block edges (64 m + 1, a partial last block, N - 1 < 64) ------------------
@pytest.mark.parametrize("n", [2, 65, 700, 2100])
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_hip_neighbors_equals_lexsort_of_the_oracle_matrix(method, n, sa, oracle):
    store, scoring, full = oracle_case(sa, oracle, method, n)
    for k in k_values(n):
        assert_same(sa.hip_neighbors(store, scoring, k), expected_neighbors(full, k), f"{method} N={n} k={k}")


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 32, 64])
def test_ties_across_the_cut(k, sa, oracle):
    """short DNA under SW / nuc44: few distinct scores, so the k-th and the (k + 1)-th best are often equal and only the
    index rule decides who is in"""
    store = sa.SequenceStore.from_sequences(make_dna_set(300, 120, 180, 4))
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    full = tri_to_full(oracle.align(store, scoring, triangular=True), store.num)
    # from the oracle's scores alone, before the device is asked: the case does test the rule
    tied = 0
    for r in range(store.num):
        best = np.sort(np.delete(full[r], r))[::-1]
        tied += best[k - 1] == best[k]
    print(f"k = {k}: {tied} of {store.num} rows have equal k-th and (k+1)-th best scores")
    assert tied >= store.num // 10
    assert_same(sa.hip_neighbors(store, scoring, k), expected_neighbors(full, k), f"ties k={k}")


@pytest.mark.parametrize("n,k", [(130, 64), (130, 5), (66, 65 - 1)])
def test_all_scores_equal(n, k, sa):
    """every sequence identical: every row must come out as 0, 1, .. without r"""
    store = sa.SequenceStore.from_sequences([b"ARNDCQEGHILKMFPSTWYV" * 2] * n)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    index, score = sa.hip_neighbors(store, scoring, k)
    for r in range(n):
        assert index[r].tolist() == [c for c in range(n) if c != r][:k], r
    assert (score == score[0, 0]).all()


# ---- 3. device-resident -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(700, 7), (700, 64), (65, 64)])
def test_context_neighbors_on_a_stream_writes_nothing_else(n, k, sa, oracle):
    import torch
    store, scoring, full = oracle_case(sa, oracle, "ga", n)
    poison, tail = -0x5A5A5A5B, 4096
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_index = torch.full((n * k + tail,), poison, dtype=torch.int32, device="cuda")
    d_score = torch.full((n * k + tail,), poison, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with sa.Context(store, scoring, 0) as ctx:
        ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=stream.cuda_stream)
        ctx.neighbors(d_packed.data_ptr(), k, d_index.data_ptr(), d_score.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
    index, score = d_index.cpu().numpy(), d_score.cpu().numpy()
    assert (index[n * k:] == poison).all() and (score[n * k:] == poison).all(), "written beyond N * k elements"
    assert_same((index[:n * k].reshape(n, k), score[:n * k].reshape(n, k)), expected_neighbors(full, k), f"device-resident N={n} k={k}")
    assert np.array_equal(tri_to_full(d_packed.cpu().numpy(), n), full)  # (the input is read only)


# ---- 4. tile jobs -----------------------------------------------------------------------------------------------------------
def test_tile_job_neighbors(sa, oracle, monkeypatch):
    n, chunk = 700, 256
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    want = {k: sa.hip_neighbors(store, scoring, k) for k in (1, 10, 64)}
    assert_same(want[10], expected_neighbors(full, 10))
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        with pytest.raises(sa.AlignError, match="not finished"):
            job.neighbors(10)  # the walk has not ended: the matrix is not there yet
        while job.next():
            pass
        for k in (1, 10, 64):
            assert_same(job.neighbors(k), want[k], f"tile job k={k}")
        with pytest.raises(sa.AlignError):
            job.neighbors(0)
    # dealt over three jobs: none of them holds the whole matrix
    monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
    with sa.DeflateJob.begin(store, scoring, chunk, level=1) as job:
        while job.next():
            pass
        with pytest.raises(sa.AlignError, match="dealt over 3 jobs"):
            job.neighbors(10)


def test_created_job_neighbors(sa, oracle):
    """sa_zjob_create over a caller's device matrix: packed -> any time; full -> refused"""
    import torch
    n = 700
    store, scoring, full = oracle_case(sa, oracle, "nw", n)
    from tests.test_gpu_deflate import packed_of
    d_packed = torch.from_numpy(packed_of(full)).cuda()
    d_full = torch.from_numpy(np.ascontiguousarray(full)).cuda()
    torch.cuda.synchronize()
    with sa.DeflateJob(n, 256, d_packed_ptr=d_packed.data_ptr()) as job:
        assert_same(job.neighbors(12), expected_neighbors(full, 12))
    with sa.DeflateJob(n, 256, d_full_ptr=d_full.data_ptr()) as job:
        with pytest.raises(sa.AlignError, match="packed"):
            job.neighbors(12)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------
def test_bad_k_raises_and_the_process_lives_on(sa, oracle):
    import torch
    n = 40
    store, scoring, full = oracle_case(sa, oracle, "sw", n)
    for k in (0, 65, n, -3):
        with pytest.raises(sa.AlignError, match="k must be in"):
            sa.hip_neighbors(store, scoring, k)
    d_packed = torch.zeros(store.pairs, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(2 * n * 64, dtype=torch.int32, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:
        for k in (0, 65, n):
            with pytest.raises(sa.AlignError, match="k must be in"):
                ctx.neighbors(d_packed.data_ptr(), k, d_out.data_ptr(), d_out.data_ptr() + 4 * n * 64)
        with pytest.raises(sa.AlignError, match="null"):
            ctx.neighbors(0, 5, d_out.data_ptr(), d_out.data_ptr() + 4 * n * 64)
    assert not d_out.cpu().numpy().any()
    assert_same(sa.hip_neighbors(store, scoring, n - 1), expected_neighbors(full, n - 1), "a valid call after the errors")


# ---- 6. scale ---------------------------------------------------------------------------------------------------------------
def test_config2_scale(sa):
    """10 000 proteins, k = 32: cross-block and indexing errors that small N cannot show.  The expectation comes from the
    GPU's own packed matrix copied to the host (pinned to the reference by test_gpu_digests.py) and NumPy -- argpartition plus
    the tie rule; the selection is the only code under test."""
    import torch
    from tests.synth import make_config
    seqs, cfg = make_config("cfg2")
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    n, k = store.num, 32
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_index = torch.empty(n * k, dtype=torch.int32, device="cuda")
    d_score = torch.empty(n * k, dtype=torch.int32, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:
        for rep in range(2):  # (the first round loads code objects and plans)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.align_range(0, store.pairs, d_packed.data_ptr())
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ctx.neighbors(d_packed.data_ptr(), k, d_index.data_ptr(), d_score.data_ptr())
            torch.cuda.synchronize()
            t2 = time.perf_counter()
    print(f"config 2: alignment {1e3 * (t1 - t0):.2f} ms, selection of k = {k}: {1e3 * (t2 - t1):.2f} ms (host clock around a synchronised call)")
    tri = d_packed.cpu().numpy()
    full = np.zeros((n, n), np.int32)
    for j in range(1, n):
        seg = tri[j * (j - 1) // 2: j * (j - 1) // 2 + j]
        full[:j, j] = seg
        full[j, :j] = seg
    np.fill_diagonal(full, np.iinfo(np.int32).min)  # (below every NW score of this store: never among the best 32 of 9 999)
    assert tri.min() > np.iinfo(np.int32).min
    index, score = np.empty((n, k), np.int32), np.empty((n, k), np.int32)
    for r in range(n):
        row = full[r]
        cand = np.argpartition(-row.astype(np.int64), k - 1)[:k]
        kth = row[cand].min()                      # the k-th best score
        above = np.flatnonzero(row > kth)          # in for certain
        level = np.flatnonzero(row == kth)         # the tie: lowest indices first
        assert r not in above and r not in level[:k - len(above)]
        above = above[np.lexsort((above, -row[above].astype(np.int64)))]
        index[r] = np.concatenate([above, level[:k - len(above)]])
        score[r] = row[index[r]]
    assert_same((d_index.cpu().numpy().reshape(n, k), d_score.cpu().numpy().reshape(n, k)), (index, score), "config 2, k = 32")


# ---- 7. the tool ------------------------------------------------------------------------------------------------------------
def test_cli_neighbors(tmp_path, sa, oracle):
    from tests.host_binding import H5DIFF, h5_matrix, h5_sequences
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_neighbors_host import h5_dataset, h5_names
    n, k = 1100, 10
    seqs = make_protein_set(n, 30, 80, 17)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    full = tri_to_full(oracle.align(store, scoring, triangular=True), n)
    want = expected_neighbors(full, k)
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F"]

    def neighbors_of(path):
        return h5_dataset(path, "neighbor_indices", (n, k)), h5_dataset(path, "neighbor_scores", (n, k))

    for name, extra, env in (("plain", [], None), ("z9", ["-z", 9], None), ("hostmatrix", [], {"SA_HOST_MATRIX": "1"})):
        without, with_k = tmp_path / f"{name}.h5", tmp_path / f"{name}_k.h5"
        run("-i", fasta, "-o", without, *flags, *extra, "-Q", env=env)
        res = run("-i", fasta, "-o", with_k, *flags, *extra, "-k", k, "-B", "-V", env=env)
        assert "neighbor selection on the device, K = 10" in res.stdout, res.stdout
        second = "second alignment pass" in res.stdout
        # one device, the tile path: the finished job is asked, nothing is aligned twice; the host-matrix path says it did
        assert second == (env is not None or sa.device_count() != 1), res.stdout
        assert h5_names(with_k) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores"}
        assert_same(neighbors_of(with_k), want, name)
        assert np.array_equal(h5_matrix(with_k, n), full) and h5_sequences(with_k) == seqs
        for dataset in ("/similarity_matrix", "/sequences"):
            diff = subprocess.run([str(H5DIFF), str(without), str(with_k), dataset], capture_output=True, text=True)
            assert diff.returncode == 0, diff.stdout + diff.stderr

    only = tmp_path / "only.h5"
    res = run("-i", fasta, "-o", only, *flags, "-k", k, "--neighbors-only", "-B")
    assert "only the neighbors come back" in res.stdout, res.stdout
    assert h5_names(only) == {"/sequences", "/neighbor_indices", "/neighbor_scores"}
    assert_same(neighbors_of(only), want, "--neighbors-only")
    assert h5_sequences(only) == seqs
    assert only.stat().st_size < (tmp_path / "plain.h5").stat().st_size // 10

    # -W: the selection still runs (for timing), nothing is written
    res = run("-i", fasta, "-W", *flags, "-k", k, "-B")
    assert "neighbor selection on the device, K = 10" in res.stdout

    for bad, message in ((["-k", 2000], "Neighbor count must be between 1-64"), (["-k", 0], "Neighbor count must be between 1-64"),
                         (["--neighbors-only"], "--neighbors-only requires -k")):
        out = tmp_path / "bad.h5"
        res = run("-i", fasta, "-o", out, *flags, *bad, check=False)
        assert res.returncode == 1 and message in res.stderr and "usage information" in res.stderr, res.stderr
        assert not out.exists()
    # K within [1, 64] but above N - 1: known only after loading (and filtering)
    few = tmp_path / "few.fasta"
    write_fasta(few, seqs[:20])
    res = run("-i", few, "-o", tmp_path / "few.h5", *flags, "-k", 20, check=False)
    assert res.returncode == 1 and "exceeds the 19 other sequences" in res.stderr, res.stderr
    run("-i", few, "-o", tmp_path / "few.h5", *flags, "-k", 19, "-Q")
    assert_same((h5_dataset(tmp_path / "few.h5", "neighbor_indices", (20, 19)), h5_dataset(tmp_path / "few.h5", "neighbor_scores", (20, 19))),
                expected_neighbors(full[:20, :20], 19), "N <= 256")
