"""GPU (-m gpu): the tool's --fit option end to end (FASTA in -> the fit sweep, the hits and the fitted alignments on the device ->
HDF5 out).  Every dataset is compared with tests/fit_ref.py (plain Python) and NumPy's lexsort, never with the library; the dataset
names are exactly the search's plus the three of --fit; a run without --fit writes none of them."""
import subprocess

import numpy as np
import pytest

from tests import fit_ref
from tests.host_binding import ROOT
from tests.search_cases import expected_hits, h5_strings
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_gpu_fit import COLUMNS, planted
from tests.test_neighbors_host import h5_names

pytestmark = pytest.mark.gpu
CLI = ROOT / "cli" / "seqalign"
N, M, K = 24, 6, 5
HIT_SETS = {"/sequences", "/query_sequences", "/hit_indices", "/hit_scores"}
FIT_SETS = {"/hit_db_begin", "/hit_db_end", "/search_ends"}
ALN_SETS = {"/hit_alignment_records", "/hit_cigar_offsets", "/hit_cigars"}
VALUE_SETS = {"/hit_values", "/hit_quantity", "/hit_scale"}


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


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """12 distinct database sequences each present twice (ties cross the cut at K = 5), 6 queries, three of them planted"""
    distinct = make_protein_set(12, 30, 90, 21)
    db = [distinct[k] for k in np.random.default_rng(6).permutation(np.repeat(np.arange(12), 2))]
    queries = make_protein_set(M, 8, 40, 22)
    for q, (src, start, length) in {0: (3, 5, 20), 2: (7, 1, 28), 5: (11, 12, 15)}.items():
        queries[q] = planted(distinct[src], start, length, 30 + q)
    where = tmp_path_factory.mktemp("fit_cli")
    write_fasta(where / "db.fasta", db)
    write_fasta(where / "q.fasta", queries)
    return where, db, queries


def rectangles(scoring, db, queries):
    res = [[fit_ref.fit_pair(scoring, d, q) for d in db] for q in queries]
    score = np.array([[r["score"] for r in row] for row in res], np.int32)
    pid = np.array([[fit_ref.pid(r["identities"], r["columns"], len(db[d]), len(queries[q]), COLUMNS) for d, r in enumerate(row)] for q, row in enumerate(res)],
                   np.int32)
    return res, score, pid


@pytest.mark.parametrize("method,flags,gaps", [("nw", ["-p", "4"], dict(gap_pen=4)), ("ga", ["-s", "10", "-e", "1"], dict(gap_open=10, gap_extend=1))])
def test_cli_fit(method, flags, gaps, case, tmp_path, sa):
    where, db, queries = case
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    res, score, pid = rectangles(scoring, db, queries)
    common = ["-i", where / "db.fasta", "-a", method, "-m", "blosum62", *flags, "-F", "-P", "--query", where / "q.fasta", "-k", K]

    # by score, with the alignments and the rectangle
    out = tmp_path / "fit.h5"
    text = run(*common, "-o", out, "--fit", "--alignments", "--query-scores").stdout
    assert "Fit: every query whole" in text
    assert h5_names(out) == HIT_SETS | FIT_SETS | ALN_SETS | {"/query_scores"}
    assert h5_strings(out, "sequences") == db and h5_strings(out, "query_sequences") == queries
    wi, ws = expected_hits(score, K)
    at = wi.astype(np.int64)
    index = h5_array(out, "hit_indices", "<i4").reshape(M, K)
    assert np.array_equal(index, wi) and np.array_equal(h5_array(out, "hit_scores", "<i4").reshape(M, K), ws)
    begin, end = h5_array(out, "hit_db_begin", "<i4").reshape(M, K), h5_array(out, "hit_db_end", "<i4").reshape(M, K)
    assert np.array_equal(begin, np.array([[res[q][d]["db_begin"] for d in at[q]] for q in range(M)]))
    assert np.array_equal(end, np.array([[res[q][d]["db_end"] for d in at[q]] for q in range(M)]))
    assert h5_array(out, "search_ends", "<i4").tolist() == [1]
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), score)
    assert (begin > 0).any() and any(end[q, t] < len(db[at[q, t]]) for q in range(M) for t in range(K))  # the overhang is there to be free
    fields = h5_array(out, "hit_alignment_records", "<i4").reshape(M * K, 8)
    offsets, cigars = h5_array(out, "hit_cigar_offsets", "<i8"), h5_array(out, "hit_cigars", "<u4")
    assert offsets[0] == 0 and offsets[-1] == cigars.size
    for t in range(M * K):
        q, d = t // K, int(at[t // K, t % K])
        want = res[q][d]
        assert fields[t].tolist() == [want["score"], 0, len(queries[q]), want["db_begin"], want["db_end"], want["columns"], want["identities"],
                                      len(want["cigar"])], f"record of hit {t % K} of query {q}"
        runs = [(int(w) >> 4, "MID"[int(w) & 15]) for w in cigars[offsets[t]:offsets[t + 1]]]
        assert runs == want["cigar"], f"CIGAR of hit {t % K} of query {q}"

    # ranked by the identity of the fitted alignment: the datasets of --hits-by beside those of --fit
    out = tmp_path / "pid.h5"
    run(*common, "-o", out, "--fit", "--hits-by", "identity-columns", "--query-scores")
    assert h5_names(out) == HIT_SETS | FIT_SETS | VALUE_SETS | {"/query_scores", "/query_values"}
    wi, wv = expected_hits(pid, K)
    at = wi.astype(np.int64)
    assert np.array_equal(h5_array(out, "hit_indices", "<i4").reshape(M, K), wi) and np.array_equal(h5_array(out, "hit_values", "<i4").reshape(M, K), wv)
    assert np.array_equal(h5_array(out, "hit_scores", "<i4").reshape(M, K), np.take_along_axis(score, at, 1))
    assert np.array_equal(h5_array(out, "hit_db_begin", "<i4").reshape(M, K), np.array([[res[q][d]["db_begin"] for d in at[q]] for q in range(M)]))
    assert np.array_equal(h5_array(out, "hit_db_end", "<i4").reshape(M, K), np.array([[res[q][d]["db_end"] for d in at[q]] for q in range(M)]))
    assert h5_array(out, "hit_quantity", "<i4").tolist() == [2, 0, COLUMNS] and h5_array(out, "hit_scale", "<i4").tolist() == [1000000]
    assert np.array_equal(h5_array(out, "query_values", "<i4").reshape(M, N), pid)
    assert np.array_equal(h5_array(out, "query_scores", "<i4").reshape(M, N), score)

    # --hits-by score is --fit alone; a run without --fit writes none of the three datasets, and other scores
    a, b = tmp_path / "a.h5", tmp_path / "b.h5"
    run(*common, "-o", a, "--fit")
    run(*common, "-o", b, "--fit", "--hits-by", "score")
    assert h5_names(a) == h5_names(b) == HIT_SETS | FIT_SETS
    for name in ("hit_indices", "hit_scores", "hit_db_begin", "hit_db_end"):
        assert np.array_equal(h5_array(a, name, "<i4"), h5_array(b, name, "<i4"))
    plain = tmp_path / "plain.h5"
    run(*common, "-o", plain)
    assert h5_names(plain) == HIT_SETS
    assert (h5_array(plain, "hit_scores", "<i4").reshape(M, K) <= h5_array(a, "hit_scores", "<i4").reshape(M, K)[:, :1]).all()
    assert (h5_array(plain, "hit_scores", "<i4") != h5_array(a, "hit_scores", "<i4")).any()
