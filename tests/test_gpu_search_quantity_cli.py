"""GPU (-m gpu): the tool's --hits-by option end to end (FASTA in -> the rectangle, the values and the hits on the device -> HDF5
out).  Every dataset equals what hip_search returns for the same stores and the same quantity, the dataset names are exactly the
search's plus the option's, and --hits-by score writes the file the tool writes without the option."""
import numpy as np
import pytest

from tests.search_cases import h5_strings
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_gpu_search_cli import ALN_SETS, FLAGS, HIT_SETS, K, M, N, built_cli, run, write_fasta  # noqa: F401  (built_cli: a fixture)
from tests.test_neighbors_host import h5_names

pytestmark = pytest.mark.gpu
VALUE_SETS = {"/hit_values", "/hit_quantity", "/hit_scale"}
DEN_SETS = {"/database_denominators", "/query_denominators"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("hits_by")
    db_seqs, query_seqs = make_protein_set(N, 20, 60, 11), make_protein_set(M, 20, 60, 12)
    write_fasta(d / "db.fasta", db_seqs)
    write_fasta(d / "q.fasta", query_seqs)
    return d, db_seqs, query_seqs


def test_hits_by_a_normalised_score(files, sa):
    d, db_seqs, query_seqs = files
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    out = d / "self-min.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--hits-by", "self-min", "--alignments", "--query-scores", "-B")
    assert "hits by self-min on the device: denominators + sweep over 6000 pairs" in res.stdout and f"hit selection on the device, K = {K}" in res.stdout, res.stdout
    assert "Hits ranked by self-min, in parts per million" in res.stdout and "Neighbors:" not in res.stdout, res.stdout
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    index, value, score, rect, vrect, den = sa.hip_search(db, queries, scoring, k=K, rect=True, norm=sa.Norm(sa.NORM_SELF, sa.NORM_MIN))
    assert h5_names(out) == HIT_SETS | ALN_SETS | VALUE_SETS | DEN_SETS | {"/query_scores", "/query_values"}
    assert h5_strings(out, "sequences") == db_seqs and h5_strings(out, "query_sequences") == query_seqs
    assert np.array_equal(h5_array(out, "hit_indices", "<i4").reshape(M, K), index)
    assert np.array_equal(h5_array(out, "hit_values", "<i4").reshape(M, K), value)
    assert np.array_equal(h5_array(out, "hit_scores", "<i4").reshape(M, K), score)
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), rect)
    assert np.array_equal(h5_array(out, "query_values", "<i4").reshape(M, N), vrect)
    assert h5_array(out, "hit_quantity", "<i4").tolist() == [1, sa.NORM_SELF, sa.NORM_MIN] and h5_array(out, "hit_scale", "<i4").tolist() == [1000000]
    assert np.array_equal(h5_array(out, "database_denominators", "<i4"), den[:N]) and np.array_equal(h5_array(out, "query_denominators", "<i4"), den[N:])
    # the values are the contract's, from the file's own raw scores and denominators
    assert all(sa.norm_value(int(rect[q, t]), int(den[t]), int(den[N + q]), sa.NORM_MIN) == int(vrect[q, t]) for q in range(M) for t in range(0, N, 37))
    # --alignments is unchanged: a = the query, b = the hit, the record's score the hit's raw score
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        alns = ctx.alignments([(N + q, int(index[q, t])) for q in range(M) for t in range(K)])
    fields = h5_array(out, "hit_alignment_records", "<i4").reshape(M * K, 8)
    for t, f in enumerate(("score", "a_begin", "a_end", "b_begin", "b_end", "columns", "identities", "cigar_len")):
        assert np.array_equal(fields[:, t], alns.records[f]), f
    assert np.array_equal(fields[:, 0], score.reshape(-1))
    assert np.array_equal(h5_array(out, "hit_cigars", "<u4"), alns.cigar)


def test_hits_by_percent_identity(files, sa):
    d, db_seqs, query_seqs = files
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    out = d / "identity.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--hits-by", "identity-columns", "-B")
    assert "hits by identity-columns on the device: one identity sweep over 6000 pairs" in res.stdout, res.stdout
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    index, value, score = sa.hip_search(db, queries, scoring, k=K, pid=sa.PID_COLUMNS)
    assert h5_names(out) == HIT_SETS | VALUE_SETS
    assert np.array_equal(h5_array(out, "hit_indices", "<i4").reshape(M, K), index)
    assert np.array_equal(h5_array(out, "hit_values", "<i4").reshape(M, K), value)
    assert np.array_equal(h5_array(out, "hit_scores", "<i4").reshape(M, K), score)
    assert h5_array(out, "hit_quantity", "<i4").tolist() == [2, 0, sa.PID_COLUMNS] and h5_array(out, "hit_scale", "<i4").tolist() == [1000000]
    assert (np.diff(value.astype(np.int64), axis=1) <= 0).all()


def test_hits_by_score_writes_the_file_of_no_option(files, sa):
    d, _, _ = files
    a, b = d / "plain.h5", d / "by-score.h5"
    plain = run("-i", d / "db.fasta", "-o", a, *FLAGS, "--query", d / "q.fasta", "-k", K, "--alignments", "--query-scores")
    by_score = run("-i", d / "db.fasta", "-o", b, *FLAGS, "--query", d / "q.fasta", "-k", K, "--alignments", "--query-scores", "--hits-by", "score")
    for res in (plain, by_score):  # the banner of a search is what it was: its queries, no neighbour selection, no quantity
        assert f"Queries: {d / 'q.fasta'}, the {K} best database sequences of each" in res.stdout, res.stdout
        assert "Neighbors:" not in res.stdout and "Hits ranked by" not in res.stdout, res.stdout
    assert plain.stdout.replace(str(a), "OUT") == by_score.stdout.replace(str(b), "OUT")
    assert h5_names(a) == h5_names(b) == HIT_SETS | ALN_SETS | {"/query_scores"}
    for name, dtype in (("hit_indices", "<i4"), ("hit_scores", "<i4"), ("query_scores", "<i4"), ("hit_alignment_records", "<i4"),
                        ("hit_cigar_offsets", "<i8"), ("hit_cigars", "<u4")):
        assert h5_array(a, name, dtype).tobytes() == h5_array(b, name, dtype).tobytes(), name
    for name in ("sequences", "query_sequences"):
        assert h5_strings(a, name) == h5_strings(b, name)
