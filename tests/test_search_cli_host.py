"""CPU: the tool's --query option where it needs no device -- the refused combinations, K above the database, --help -- and its one
writer, sa_host_write_search of cli/libsa_host.so, through ctypes: /sequences, /query_sequences, /hit_indices, /hit_scores, with a
rectangle /query_scores, with records /hit_alignment_records, /hit_cigar_offsets and /hit_cigars; never /similarity_matrix."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.host_binding import ROOT, Host, HostError, _Store
from tests.search_cases import h5_strings
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_neighbors_host import h5_names

ALN = np.dtype([("score", "<i4"), ("a_begin", "<i4"), ("a_end", "<i4"), ("b_begin", "<i4"), ("b_end", "<i4"),
                ("columns", "<i4"), ("identities", "<i4"), ("cigar_len", "<i4"), ("cigar_off", "<i8")])  # struct sa_aln


@pytest.fixture(scope="module")
def cli():
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return exe


# ---- the tool ----------------------------------------------------------------------------------------------------------------
REFUSED = [
    (["--query-scores"], "--query-scores requires --query"),
    (["--query", "Q"], "--query requires -k"),
    (["--query", "Q", "-k", "2", "--neighbors-only"], "--query and --neighbors-only conflict"),
    (["--query", "Q", "-k", "2", "--min-score", "5"], "--query and --min-score conflict"),
    (["--query", "Q", "-k", "2", "--min-score", "5", "--edges-only"], "--query and --edges-only conflict"),
    (["--query", "Q", "-k", "2", "--min-quantile", "0.9"], "--query and --min-quantile conflict"),
    (["--query", "Q", "-k", "2", "--linkage"], "--query and --linkage conflict"),
    (["--query", "Q", "-k", "2", "--linkage-only"], "--query and --linkage-only conflict"),
    (["--query", "Q", "-k", "2", "--linkage", "--linkage-method", "complete"], "--query and --linkage-method conflict"),
    (["--query", "Q", "-k", "2", "--clusters", "5"], "--query and --clusters conflict"),
    (["--query", "Q", "-k", "2", "--clusters-quantile", "0.5"], "--query and --clusters-quantile conflict"),
    (["--query", "Q", "-k", "2", "--quantiles", "0.5,0.9"], "--query and --quantiles conflict"),
    (["--query", "Q", "-k", "2", "--normalize", "self-min"], "--query and --normalize conflict"),
    (["--query", "Q", "-k", "2", "--identity", "columns"], "--query and --identity conflict"),
    (["--query", "Q", "-k", "2", "-z", "3"], "--query and -z, --compression conflict"),
    (["--query", "Q", "-k", "4"], "Hit count 4 exceeds the 3 database sequences"),  # (known once the database is loaded)
    (["--query", "Q", "-k", "65"], "Neighbor count must be between 1-64"),
]


@pytest.mark.parametrize("bad,message", REFUSED)
def test_refused_with_a_message_and_no_output(bad, message, cli, tmp_path):
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nARNDCQEG\n>b\nARNDCQEGHIL\n>c\nHILKMFPSTW\n")
    queries.write_bytes(b">x\nARNDCQ\n>y\nHILKMF\n")
    bad = [str(queries) if word == "Q" else word for word in bad]
    res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-a", "nw", "-m", "blosum62", "-p", "4", "-F", "-P", *bad],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and message in res.stderr and "usage information" in res.stderr, res.stdout + res.stderr
    assert not out.exists()


def test_a_query_file_goes_through_the_input_reader(cli, tmp_path):
    """same reader, same residue check: a query with a letter outside the matrix is the reader's error, before any device"""
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nARNDCQEG\n>b\nARNDCQEGHIL\n>c\nHILKMFPSTW\n")
    for body in (b">x\nARND1CQ\n>y\nHILKMF\n", b""):
        queries.write_bytes(body)
        res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-a", "nw", "-m", "blosum62", "-p", "4", "-F", "-P",
                              "--query", str(queries), "-k", "2"], capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and "error:" in res.stderr, res.stdout + res.stderr
        assert not out.exists()
    res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-a", "nw", "-m", "blosum62", "-p", "4", "-F", "-P",
                          "--query", str(tmp_path / "missing.fasta"), "-k", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "Failed to open missing.fasta" in res.stderr, res.stderr


def test_help_documents_the_search(cli):
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--query FILE", "--query-scores", "/query_sequences", "/hit_indices", "/hit_scores", "/hit_alignment_records",
                 "/hit_cigar_offsets", "/hit_cigars", "/query_scores", "no /similarity_matrix", "never the queries"):
        assert word in text, word


# ---- the writer --------------------------------------------------------------------------------------------------------------
class SearchHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_search.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        self.lib.sa_host_write_search.restype = C.c_int

    def write_search(self, path, db, queries, lut, k, index, score, rect=None, records=None, cigar=None):
        sd = self.parse(b"".join(b">s\n" + s + b"\n" for s in db), "fasta", lut)
        sq = self.parse(b"".join(b">s\n" + s + b"\n" for s in queries), "fasta", lut)
        try:
            index, score = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(score, np.int32)
            rect = None if rect is None else np.ascontiguousarray(rect, np.int32)
            cigar = None if cigar is None else np.ascontiguousarray(cigar, np.uint32)
            ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
            if self.lib.sa_host_write_search(str(path).encode(), C.byref(sd), C.byref(sq), int(k), index.ctypes.data, score.ctypes.data,
                                             ptr(rect), None if records is None else records.ctypes.data, ptr(cigar),
                                             0 if cigar is None else cigar.size):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(sd))
            self.lib.sa_host_store_free(C.byref(sq))


@pytest.fixture(scope="module")
def host():
    return SearchHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, m, k, seed):
    rng = np.random.default_rng(seed)
    db, queries = make_protein_set(n, 8, 30, seed), make_protein_set(m, 8, 30, seed + 1)
    index = np.stack([rng.permutation(n)[:k] for _ in range(m)]).astype(np.int32)
    score = rng.integers(-500, 500, (m, k)).astype(np.int32)
    rect = rng.integers(-2**31, 2**31 - 1, (m, n), dtype=np.int64).astype(np.int32)
    records = np.zeros(m * k, ALN)
    for f in ALN.names[:7]:
        records[f] = rng.integers(0, 1000, m * k)
    records["cigar_len"] = rng.integers(0, 4, m * k)
    records["cigar_off"] = np.concatenate([[0], np.cumsum(records["cigar_len"])[:-1]])
    cigar = rng.integers(0, 2**32 - 1, int(records["cigar_len"].sum()), dtype=np.int64).astype(np.uint32)
    return db, queries, index, score, rect, records, cigar


@pytest.mark.parametrize("n,m,k", [(40, 7, 3), (2, 2, 2), (300, 20, 64)])
def test_hits_alone(n, m, k, host, protein_lut, tmp_path):
    db, queries, index, score, _, _, _ = case(n, m, k, 5)
    path = tmp_path / "s.h5"
    host.write_search(path, db, queries, protein_lut, k, index, score)
    assert h5_names(path) == {"/sequences", "/query_sequences", "/hit_indices", "/hit_scores"}
    assert h5_strings(path, "sequences") == db and h5_strings(path, "query_sequences") == queries
    assert np.array_equal(h5_array(path, "hit_indices", "<i4").reshape(m, k), index)
    assert np.array_equal(h5_array(path, "hit_scores", "<i4").reshape(m, k), score)


def test_everything(host, protein_lut, tmp_path):
    n, m, k = 40, 7, 3
    db, queries, index, score, rect, records, cigar = case(n, m, k, 6)
    path = tmp_path / "s.h5"
    host.write_search(path, db, queries, protein_lut, k, index, score, rect, records, cigar)
    assert h5_names(path) == {"/sequences", "/query_sequences", "/hit_indices", "/hit_scores", "/query_scores", "/hit_alignment_records",
                              "/hit_cigar_offsets", "/hit_cigars"}
    assert np.array_equal(h5_array(path, "query_scores", "<i4").reshape(m, n), rect)
    fields = h5_array(path, "hit_alignment_records", "<i4").reshape(m * k, 8)
    for t, f in enumerate(ALN.names[:8]):
        assert np.array_equal(fields[:, t], records[f]), f
    assert np.array_equal(h5_array(path, "hit_cigar_offsets", "<i8"), np.concatenate([records["cigar_off"], [cigar.size]]))
    assert np.array_equal(h5_array(path, "hit_cigars", "<u4"), cigar)
    assert h5_strings(path, "sequences") == db and h5_strings(path, "query_sequences") == queries


def test_records_without_a_single_run(host, protein_lut, tmp_path):
    """(local alignments may all be empty): the three datasets are there, /hit_cigars with extent 0"""
    db, queries, index, score, _, records, _ = case(10, 3, 2, 7)
    records["cigar_len"], records["cigar_off"] = 0, 0
    path = tmp_path / "s.h5"
    host.write_search(path, db, queries, protein_lut, 2, index, score, None, records, np.zeros(0, np.uint32))
    assert {"/hit_alignment_records", "/hit_cigar_offsets", "/hit_cigars"} <= h5_names(path) and "/query_scores" not in h5_names(path)
    assert h5_array(path, "hit_cigars", "<u4").size == 0 and not h5_array(path, "hit_cigar_offsets", "<i8").any()


@pytest.mark.parametrize("k", [0, -1, 65, 11])
def test_bad_k_is_an_error_and_no_file(k, host, protein_lut, tmp_path):
    db, queries, index, score, _, _, _ = case(10, 3, 2, 8)
    path = tmp_path / "s.h5"
    with pytest.raises(HostError, match="Hit count must be between 1 and 64"):
        host.write_search(path, db, queries, protein_lut, k, np.zeros((3, 70), np.int32), np.zeros((3, 70), np.int32))
    assert not path.exists()


@pytest.mark.parametrize("wrong", [-1, 10, 2**31 - 1])
def test_an_index_outside_the_database_is_an_error_and_no_file(wrong, host, protein_lut, tmp_path):
    db, queries, index, score, _, _, _ = case(10, 3, 2, 9)
    index[2, 1] = wrong
    path = tmp_path / "s.h5"
    with pytest.raises(HostError, match="outside the 10 database sequences"):
        host.write_search(path, db, queries, protein_lut, 2, index, score)
    assert not path.exists()
