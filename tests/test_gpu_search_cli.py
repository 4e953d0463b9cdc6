"""GPU (-m gpu): the tool's --query option end to end (FASTA in -> the M x N rectangle and the hits on the device -> HDF5 out).
Every dataset equals what hip_search and SearchContext.alignments return for the same stores, and /query_scores also the oracle's
rectangle; the dataset names are exactly the search's, /similarity_matrix is absent; with -f the hits refer to the filtered
/sequences; a refused combination exits with its message."""
import subprocess

import numpy as np
import pytest

from tests.host_binding import ROOT
from tests.search_cases import expected_hits, h5_strings, oracle_rect
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_neighbors_host import h5_names

pytestmark = pytest.mark.gpu
CLI = ROOT / "cli" / "seqalign"
N, M, K = 300, 20, 3
FLAGS = ["-a", "nw", "-m", "blosum62", "-p", "4", "-F", "-P"]
HIT_SETS = {"/sequences", "/query_sequences", "/hit_indices", "/hit_scores"}
ALN_SETS = {"/hit_alignment_records", "/hit_cigar_offsets", "/hit_cigars"}


@pytest.fixture(scope="module", autouse=True)
def built_cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])


def run(*args, check=True):
    res = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=600)
    if check:
        assert res.returncode == 0, res.stdout + res.stderr
    return res


def write_fasta(path, seqs):
    path.write_bytes(b"".join(b">seq%d\n" % k + s[:60] + b"\n" + s[60:] + b"\n" for k, s in enumerate(seqs)))


def same_as_the_library(path, sa, oracle, db_seqs, query_seqs, scoring, with_rect=True):
    """every dataset of a --query -k K --alignments [--query-scores] file against the library's own calls"""
    n, m = len(db_seqs), len(query_seqs)
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    index, score, rect = sa.hip_search(db, queries, scoring, k=K, rect=True)
    want = oracle_rect(sa, oracle, db_seqs, query_seqs, scoring)
    assert np.array_equal(rect, want)
    assert h5_names(path) == HIT_SETS | ALN_SETS | ({"/query_scores"} if with_rect else set())
    assert h5_strings(path, "sequences") == db_seqs and h5_strings(path, "query_sequences") == query_seqs
    got_index, got_score = h5_array(path, "hit_indices", "<i4").reshape(m, K), h5_array(path, "hit_scores", "<i4").reshape(m, K)
    assert np.array_equal(got_index, index) and np.array_equal(got_score, score)
    wi, ws = expected_hits(want, K)
    assert np.array_equal(got_index, wi) and np.array_equal(got_score, ws)
    if with_rect:
        assert np.array_equal(h5_array(path, "query_scores", "<i4").reshape(m, n), want)
    with sa.SearchContext(db, queries, scoring, 0) as ctx:
        alns = ctx.alignments([(n + q, int(index[q, t])) for q in range(m) for t in range(K)])
    fields = h5_array(path, "hit_alignment_records", "<i4").reshape(m * K, 8)
    for t, f in enumerate(("score", "a_begin", "a_end", "b_begin", "b_end", "columns", "identities", "cigar_len")):
        assert np.array_equal(fields[:, t], alns.records[f]), f
    assert np.array_equal(fields[:, 0], score.reshape(-1))  # a record's score is the hit's
    assert np.array_equal(h5_array(path, "hit_cigar_offsets", "<i8"), np.concatenate([alns.records["cigar_off"], [alns.cigar.size]]))
    assert np.array_equal(h5_array(path, "hit_cigars", "<u4"), alns.cigar)


def test_cli_search(tmp_path, sa, oracle):
    db_seqs, query_seqs = make_protein_set(N, 20, 60, 11), make_protein_set(M, 20, 60, 12)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    fasta, qfasta, out = tmp_path / "db.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    write_fasta(fasta, db_seqs)
    write_fasta(qfasta, query_seqs)
    res = run("-i", fasta, "-o", out, *FLAGS, "--query", qfasta, "-k", K, "--alignments", "--query-scores", "-B")
    assert f"hit selection on the device, K = {K}" in res.stdout and f"alignments of the {M * K} hit pairs" in res.stdout, res.stdout
    assert f"Performing {M * N} pairwise alignments" in res.stdout, res.stdout  # (the rectangle, not a triangle)
    same_as_the_library(out, sa, oracle, db_seqs, query_seqs, scoring)

    # the hits alone: four datasets
    plain = tmp_path / "plain.h5"
    run("-i", fasta, "-o", plain, *FLAGS, "--query", qfasta, "-k", K, "-Q")
    assert h5_names(plain) == HIT_SETS
    assert np.array_equal(h5_array(plain, "hit_indices", "<i4"), h5_array(out, "hit_indices", "<i4"))

    # one refused combination: its message, exit code 1, no file
    bad = tmp_path / "bad.h5"
    res = run("-i", fasta, "-o", bad, *FLAGS, "--query", qfasta, "-k", K, "--linkage", check=False)
    assert res.returncode == 1 and "--query and --linkage conflict" in res.stderr and "usage information" in res.stderr, res.stderr
    assert not bad.exists()


def test_cli_search_filters_the_database_only(tmp_path, sa, oracle):
    """-f 0.9 on a database with planted duplicates: they leave /sequences, and the hit indices refer to what is left; queries that
    are duplicates of each other (and of database sequences) all stay"""
    base = make_protein_set(N, 20, 60, 11)
    db_seqs = list(base)
    planted = {50: 3, 120: 7, 299: 100}
    for at, of in planted.items():
        db_seqs[at] = base[of]
    kept = [s for k, s in enumerate(db_seqs) if k not in planted]
    query_seqs = make_protein_set(M - 3, 20, 60, 12) + [base[3], base[3], base[100]]
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    fasta, qfasta, out = tmp_path / "db.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    write_fasta(fasta, db_seqs)
    write_fasta(qfasta, query_seqs)
    res = run("-i", fasta, "-o", out, *FLAGS, "--query", qfasta, "-k", K, "--alignments", "--query-scores", "-f", 0.9)
    assert "Filtered out 3 sequences" in res.stdout, res.stdout
    same_as_the_library(out, sa, oracle, kept, query_seqs, scoring)
    # the query that is database sequence 3 finds it first, under its index in the filtered /sequences (3: nothing before it left)
    assert h5_array(out, "hit_indices", "<i4").reshape(M, K)[M - 3, 0] == 3
    # ... and the one that is database sequence 100 under 99: sequence 50 before it was filtered out
    assert h5_array(out, "hit_indices", "<i4").reshape(M, K)[M - 1, 0] == 99
