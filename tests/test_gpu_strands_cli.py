"""GPU (-m gpu): the tool's --strands option end to end (FASTA in -> both strands on the device, folded -> HDF5 out), under -k,
--hits-by identity-shorter, --hits-min, --alignments and --query-scores.  Every new dataset is read back with h5dump and compared
with the expectation of tests/strands_cases.py, which never comes from the code under test: the oracle's rectangles of the queries
and of their reverse complements (rc written in Python), folded by NumPy.  --strands forward and no option write equal files."""
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF
from tests.search_cases import h5_strings
from tests.strands_cases import Folded, assert_not_degenerate, dna_database, dna_queries, folded_case, rc
from tests.test_edges_host import h5_array
from tests.test_gpu_search_cli import ALN_SETS, HIT_SETS, built_cli, run, write_fasta  # noqa: F401  (built_cli: a fixture)
from tests.test_neighbors_host import h5_names

pytestmark = pytest.mark.gpu
N, M, K = 130, 7, 9
FLAGS = ["-a", "sw", "-m", "nuc44", "-s", "10", "-e", "1", "-F", "-P"]
LIST_SETS = {"/sequences", "/query_sequences", "/hitlist_offsets", "/hitlist_indices", "/hitlist_scores", "/hitlist_min"}
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end", "columns", "identities", "cigar_len")


@pytest.fixture(scope="module")
def files(tmp_path_factory, sa, oracle):
    d = tmp_path_factory.mktemp("strands")
    db_seqs = dna_database(N, seed=701)
    query_seqs = dna_queries(db_seqs, M, seed=702)
    write_fasta(d / "db.fasta", db_seqs)
    write_fasta(d / "q.fasta", query_seqs)
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    exp = folded_case(sa, oracle, db_seqs, query_seqs, scoring)
    assert_not_degenerate(exp, K, 2, "the tool's case")
    return d, db_seqs, query_seqs, scoring, exp


def test_top_k_with_alignments_and_query_scores(files, sa):
    d, db_seqs, query_seqs, scoring, exp = files
    out = d / "topk.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--strands", "both", "--alignments", "--query-scores", "-B")
    assert "Strands: both" in res.stdout and "both strands searched" in res.stdout and "fold + strands of the hits on the device" in res.stdout, res.stdout
    assert f"Performing {2 * M * N} pairwise alignments" in res.stdout, res.stdout
    assert h5_names(out) == HIT_SETS | ALN_SETS | {"/query_scores", "/hit_strands", "/query_strands"}
    assert h5_strings(out, "sequences") == db_seqs and h5_strings(out, "query_sequences") == query_seqs  # (the queries as given)
    index, value, score, strand = exp.hits(K)
    assert np.array_equal(h5_array(out, "hit_indices", "<i4").reshape(M, K), index)
    assert np.array_equal(h5_array(out, "hit_scores", "<i4").reshape(M, K), score)
    assert np.array_equal(h5_array(out, "hit_strands", "u1").reshape(M, K), strand)
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), exp.best)
    assert np.array_equal(h5_array(out, "query_strands", "u1").reshape(M, N), exp.strand.astype(np.uint8))
    # every hit traced on its own strand: the record's score is the folded score, and the records are those of the rows N + strand M + q
    fields = h5_array(out, "hit_alignment_records", "<i4").reshape(M * K, 8)
    assert np.array_equal(fields[:, 0].reshape(M, K), score)
    cat = sa.SequenceStore.from_sequences(db_seqs + query_seqs + [rc(q) for q in query_seqs])
    alns = sa.hip_alignments(cat, scoring, [(N + int(strand[q, t]) * M + q, int(index[q, t])) for q in range(M) for t in range(K)])
    for t, f in enumerate(FIELDS):
        assert np.array_equal(fields[:, t], alns.records[f]), f
    assert np.array_equal(h5_array(out, "hit_cigars", "<u4"), alns.cigar)


def test_by_identity_shorter(files, sa):
    d, db_seqs, query_seqs, scoring, exp = files
    cat = sa.SequenceStore.from_sequences(db_seqs + query_seqs + [rc(q) for q in query_seqs])
    at = np.array([[(N + q) * (N + q - 1) // 2 + dd for dd in range(N)] for q in range(2 * M)], np.int64)
    pid = np.ascontiguousarray(sa.hip_identity(cat, scoring, denom=sa.PID_SHORTER, identities=False, columns=False)[2][at])  # (pinned by tests/test_gpu_identity.py)
    vexp = Folded(exp.fwd, exp.rev, pid[:M], pid[M:])
    assert_not_degenerate(vexp, K, 2, "by identity")
    out = d / "identity.h5"
    run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--strands", "both", "--hits-by", "identity-shorter", "--query-scores", "-Q")
    assert h5_names(out) == HIT_SETS | {"/hit_values", "/hit_quantity", "/hit_scale", "/query_scores", "/query_values", "/hit_strands", "/query_strands"}
    index, value, score, strand = vexp.hits(K)
    for name, want, dt in (("hit_indices", index, "<i4"), ("hit_values", value, "<i4"), ("hit_scores", score, "<i4"), ("hit_strands", strand, "u1")):
        assert np.array_equal(h5_array(out, name, dt).reshape(M, K), want), name
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), vexp.best)
    assert np.array_equal(h5_array(out, "query_values", "<i4").reshape(M, N), vexp.vbest)
    assert np.array_equal(h5_array(out, "query_strands", "u1").reshape(M, N), vexp.strand.astype(np.uint8))
    # a normalised kind: the denominators of the queries as given, and those of the reverse complements beside them
    out = d / "len-min.h5"
    run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "-k", K, "--strands", "both", "--hits-by", "len-min", "-Q")
    assert h5_names(out) == HIT_SETS | {"/hit_values", "/hit_quantity", "/hit_scale", "/database_denominators", "/query_denominators", "/hit_strands",
                                        "/query_reverse_denominators"}
    assert h5_array(out, "query_denominators", "<i4").tolist() == [len(q) for q in query_seqs]
    assert h5_array(out, "query_reverse_denominators", "<i4").tolist() == [len(q) for q in query_seqs]


def test_hits_min_with_alignments_and_query_scores(files, sa):
    d, db_seqs, query_seqs, scoring, exp = files
    t = int(np.sort(exp.best.reshape(-1))[exp.best.size * 9 // 10])
    offsets, index, value, score, strand = exp.above(t)
    e = int(offsets[-1])
    assert 0 < e < M * N and {0, 1} <= set(strand.tolist())
    out = d / "list.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-min", t, "--strands", "both", "--alignments", "--query-scores", "-B")
    assert f"hits at or above {t} on the device: {e} hits" in res.stdout and "both strands searched" in res.stdout, res.stdout
    assert h5_names(out) == LIST_SETS | {"/hitlist_alignment_records", "/hitlist_cigar_offsets", "/hitlist_cigars", "/query_scores", "/hitlist_strands",
                                         "/query_strands"}
    assert np.array_equal(h5_array(out, "hitlist_offsets", "<i8"), offsets) and np.array_equal(h5_array(out, "hitlist_indices", "<i4"), index)
    assert np.array_equal(h5_array(out, "hitlist_scores", "<i4"), score) and np.array_equal(h5_array(out, "hitlist_strands", "u1"), strand)
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), exp.best)
    assert np.array_equal(h5_array(out, "query_strands", "u1").reshape(M, N), exp.strand.astype(np.uint8))
    fields = h5_array(out, "hitlist_alignment_records", "<i4").reshape(e, 8)
    assert np.array_equal(fields[:, 0], score)  # every hit traced on its own strand
    # a threshold above every value: a valid file with no hit and an empty /hitlist_strands
    out = d / "none.h5"
    run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", "--hits-min", 2**31 - 1, "--strands", "both", "-Q")
    assert h5_names(out) == LIST_SETS | {"/hitlist_strands"}
    assert h5_array(out, "hitlist_offsets", "<i8").tolist() == [0] * (M + 1) and h5_array(out, "hitlist_strands", "u1").size == 0


@pytest.mark.parametrize("extra", [["-k", K, "--alignments", "--query-scores"], ["-k", K, "--hits-by", "identity-shorter"], ["--hits-min", 40]],
                         ids=["top-k", "identity", "hits-min"])
def test_forward_writes_the_bytes_of_no_option(extra, files):
    d = files[0]
    plain, forward = d / "plain.h5", d / "forward.h5"
    for out, more in ((plain, []), (forward, ["--strands", "forward"])):
        if out.exists():
            out.unlink()
        run("-i", d / "db.fasta", "-o", out, *FLAGS, "--query", d / "q.fasta", *extra, *more, "-Q")
    res = subprocess.run([str(H5DIFF), str(plain), str(forward)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "", res.stdout + res.stderr
    assert h5_names(plain) == h5_names(forward) and not any("strand" in name for name in h5_names(forward))


def test_refusals_with_a_device(files):
    d = files[0]
    (d / "bad.fasta").write_bytes(b">x\nACGTACGT\n>y\nACGTUACGT\n")  # nuc44 reads no U: the loader refuses it before the strands are asked
    (d / "protein.fasta").write_bytes(b">x\nACGT\n")
    out = d / "refused.h5"
    res = run("-i", d / "db.fasta", "-o", out, *FLAGS, "-k", 2, "--strands", "both", check=False)
    assert res.returncode == 1 and "--strands both requires --query" in res.stderr and not out.exists()
    res = run("-i", d / "db.fasta", "-o", out, "-a", "sw", "-m", "blosum62", "-s", "10", "-e", "1", "-F", "-P", "--query", d / "protein.fasta", "-k", 2,
              "--strands", "both", check=False)
    assert res.returncode == 1 and "--strands both and -m blosum62 conflict" in res.stderr and not out.exists()
