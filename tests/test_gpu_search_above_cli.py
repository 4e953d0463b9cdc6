"""GPU (-m gpu): the tool's --hits-min option end to end (FASTA in -> the rectangle, the values and the hit list on the device ->
HDF5 out).  Every dataset equals what hip_search_above returns for the same stores, threshold and quantity -- and the hit list itself
is np.nonzero(values >= T) of the rectangle --query-scores writes; the dataset names are exactly the option's; and a -k search of the
same inputs still writes the library's top-k arrays, dataset for dataset, as it did before the option existed."""
import numpy as np
import pytest

from tests.search_cases import h5_strings
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_gpu_search_cli import ALN_SETS, FLAGS, HIT_SETS, K, M, N, built_cli, run, write_fasta  # noqa: F401  (built_cli: a fixture)
from tests.test_neighbors_host import h5_names

pytestmark = pytest.mark.gpu
LIST_SETS = {"/sequences", "/query_sequences", "/hitlist_offsets", "/hitlist_indices", "/hitlist_scores", "/hitlist_min"}
LIST_ALN_SETS = {"/hitlist_alignment_records", "/hitlist_cigar_offsets", "/hitlist_cigars"}
VALUE_SETS = {"/hitlist_values", "/hit_quantity", "/hit_scale"}


@pytest.fixture(scope="module")
def files(tmp_path_factory, sa):
    d = tmp_path_factory.mktemp("hits_min")
    db_seqs, query_seqs = make_protein_set(N, 20, 60, 11), make_protein_set(M, 20, 60, 12)
    write_fasta(d / "db.fasta", db_seqs)
    write_fasta(d / "q.fasta", query_seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    return d, db_seqs, query_seqs, sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring


def same_list(path, got, t):
    assert np.array_equal(h5_array(path, "hitlist_offsets", "<i8"), got.offsets)
    assert np.array_equal(h5_array(path, "hitlist_indices", "<i4"), got.index)
    assert np.array_equal(h5_array(path, "hitlist_scores", "<i4"), got.score)
    assert h5_array(path, "hitlist_min", "<i4").tolist() == [t]


def test_plain_and_with_query_scores(files, sa):
    d, db_seqs, query_seqs, db, queries, scoring = files
    rect = sa.hip_search(db, queries, scoring, rect=True)
    t = int(np.quantile(rect, 0.98))
    got = sa.hip_search_above(db, queries, scoring, t)
    assert 0 < len(got) < M * N // 10
    out = d / "plain.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-min", t, "-B")
    assert f"hits at or above {t} on the device: {len(got)} hits, count + scan + fill" in res.stdout, res.stdout
    assert f"every database sequence that scores at least {t}" in res.stdout and "best database sequences" not in res.stdout, res.stdout
    assert f"Performing {M * N} pairwise alignments" in res.stdout and "second alignment" not in res.stdout, res.stdout
    assert h5_names(out) == LIST_SETS
    assert h5_strings(out, "sequences") == db_seqs and h5_strings(out, "query_sequences") == query_seqs
    same_list(out, got, t)
    # --query-scores: the rectangle beside the list (a second alignment, said so in -B), and the list is the rectangle's
    out = d / "scores.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-min", t, "--query-scores", "-B")
    assert "a second alignment of the rectangle" in res.stdout, res.stdout
    assert h5_names(out) == LIST_SETS | {"/query_scores"}
    same_list(out, got, t)
    written = h5_array(out, "query_scores", "<i4").reshape(M, N)
    assert np.array_equal(written, rect)
    rows, cols = np.nonzero(written >= t)
    assert np.array_equal(h5_array(out, "hitlist_indices", "<i4"), cols.astype(np.int32))
    assert np.array_equal(h5_array(out, "hitlist_offsets", "<i8"), np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M))]))
    assert np.array_equal(h5_array(out, "hitlist_scores", "<i4"), written[rows, cols])
    # a threshold above every score: a valid file with no hit
    out = d / "none.h5"
    run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-min", 2**31 - 1, "--alignments", "-Q")
    assert h5_names(out) == LIST_SETS | LIST_ALN_SETS
    assert h5_array(out, "hitlist_offsets", "<i8").tolist() == [0] * (M + 1) and h5_array(out, "hitlist_indices", "<i4").size == 0
    assert h5_array(out, "hitlist_cigar_offsets", "<i8").tolist() == [0] and h5_array(out, "hitlist_alignment_records", "<i4").size == 0


def test_by_percent_identity(files, sa):
    d, db_seqs, query_seqs, db, queries, scoring = files
    rect, vrect = sa.hip_search(db, queries, scoring, rect=True, pid=sa.PID_SHORTER)
    t = int(np.quantile(vrect, 0.98))
    got = sa.hip_search_above(db, queries, scoring, t, pid=sa.PID_SHORTER)
    assert 0 < len(got) < M * N // 10
    out = d / "identity.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-by", "identity-shorter", "--hits-min", t, "--query-scores", "-B")
    assert f"whose identity-shorter is at least {t} parts per million" in res.stdout, res.stdout
    assert "hits by identity-shorter on the device: one identity sweep over 6000 pairs" in res.stdout, res.stdout
    assert h5_names(out) == LIST_SETS | VALUE_SETS | {"/query_scores", "/query_values"}
    same_list(out, got, t)
    assert np.array_equal(h5_array(out, "hitlist_values", "<i4"), got.value)
    assert h5_array(out, "hit_quantity", "<i4").tolist() == [2, 0, sa.PID_SHORTER] and h5_array(out, "hit_scale", "<i4").tolist() == [1000000]
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), rect)
    written = h5_array(out, "query_values", "<i4").reshape(M, N)
    assert np.array_equal(written, vrect)
    rows, cols = np.nonzero(written >= t)
    assert np.array_equal(got.index, cols.astype(np.int32)) and np.array_equal(got.value, written[rows, cols]) and np.array_equal(got.score, rect[rows, cols])
    # a normalised kind: the denominators as --hits-by writes them
    out = d / "self-min.h5"
    norm = sa.Norm(sa.NORM_SELF, sa.NORM_MIN)
    t = 400000
    got = sa.hip_search_above(db, queries, scoring, t, norm=norm)
    run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-by", "self-min", "--hits-min", t, "-Q")
    assert h5_names(out) == LIST_SETS | VALUE_SETS | {"/database_denominators", "/query_denominators"}
    same_list(out, got, t)
    assert np.array_equal(h5_array(out, "hitlist_values", "<i4"), got.value)
    assert h5_array(out, "hit_quantity", "<i4").tolist() == [1, sa.NORM_SELF, sa.NORM_MIN]
    assert np.array_equal(h5_array(out, "database_denominators", "<i4"), got.denominators[:N])
    assert np.array_equal(h5_array(out, "query_denominators", "<i4"), got.denominators[N:])


def test_with_alignments(files, sa):
    d, db_seqs, query_seqs, db, queries, scoring = files
    rect = sa.hip_search(db, queries, scoring, rect=True)
    t = int(np.quantile(rect, 0.98))
    got = sa.hip_search_above(db, queries, scoring, t)
    e = len(got)
    out = d / "alignments.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-min", t, "--alignments", "-B")
    assert f"alignments of the {e} hit pairs" in res.stdout, res.stdout
    assert h5_names(out) == LIST_SETS | LIST_ALN_SETS
    same_list(out, got, t)
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        alns = ctx.alignments([(N + q, int(b)) for q in range(M) for b in got.index[got.row(q)]])
    fields = h5_array(out, "hitlist_alignment_records", "<i4").reshape(e, 8)
    for k, f in enumerate(("score", "a_begin", "a_end", "b_begin", "b_end", "columns", "identities", "cigar_len")):
        assert np.array_equal(fields[:, k], alns.records[f]), f
    assert np.array_equal(fields[:, 0], got.score)  # a record's score is the hit's raw score
    assert np.array_equal(h5_array(out, "hitlist_cigar_offsets", "<i8"), np.concatenate([alns.records["cigar_off"], [alns.cigar.size]]))
    assert np.array_equal(h5_array(out, "hitlist_cigars", "<u4"), alns.cigar)


def test_a_top_k_search_writes_what_it_wrote(files, sa):
    """-k beside the new option's code: the file of a top-k search, dataset for dataset the library's top-k arrays and nothing else"""
    d, db_seqs, query_seqs, db, queries, scoring = files
    out = d / "topk.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--alignments", "--query-scores", "-B")
    assert f"Queries: {d / 'q.fasta'}, the {K} best database sequences of each" in res.stdout and "hits at or above" not in res.stdout, res.stdout
    assert f"hit selection on the device, K = {K}" in res.stdout and f"alignments of the {M * K} hit pairs" in res.stdout, res.stdout
    index, score, rect = sa.hip_search(db, queries, scoring, k=K, rect=True)
    assert h5_names(out) == HIT_SETS | ALN_SETS | {"/query_scores"}
    assert h5_strings(out, "sequences") == db_seqs and h5_strings(out, "query_sequences") == query_seqs
    assert h5_array(out, "hit_indices", "<i4").tobytes() == index.astype("<i4").tobytes()
    assert h5_array(out, "hit_scores", "<i4").tobytes() == score.astype("<i4").tobytes()
    assert h5_array(out, "query_scores", "<i4").tobytes() == rect.astype("<i4").tobytes()
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        alns = ctx.alignments([(N + q, int(index[q, t])) for q in range(M) for t in range(K)])
    fields = h5_array(out, "hit_alignment_records", "<i4").reshape(M * K, 8)
    for k, f in enumerate(("score", "a_begin", "a_end", "b_begin", "b_end", "columns", "identities", "cigar_len")):
        assert np.array_equal(fields[:, k], alns.records[f]), f
    assert np.array_equal(h5_array(out, "hit_cigar_offsets", "<i8"), np.concatenate([alns.records["cigar_off"], [alns.cigar.size]]))
    assert h5_array(out, "hit_cigars", "<u4").tobytes() == alns.cigar.astype("<u4").tobytes()
    # with a quantity as well
    out = d / "topk-by.h5"
    run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--hits-by", "identity-shorter", "-Q")
    index, value, score = sa.hip_search(db, queries, scoring, k=K, pid=sa.PID_SHORTER)
    assert h5_names(out) == HIT_SETS | {"/hit_values", "/hit_quantity", "/hit_scale"}
    for name, want in (("hit_indices", index), ("hit_values", value), ("hit_scores", score)):
        assert h5_array(out, name, "<i4").tobytes() == want.astype("<i4").tobytes(), name
