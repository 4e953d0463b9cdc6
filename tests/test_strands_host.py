"""CPU: what the two-strand search (csrc/sa_strands.hip, --strands) needs no device for.
  - Every refusal of sa_hip_search_strands / sa_hip_search_above_strands / sa_ctx_create_search_strands that comes before a device is
    looked for, with its message, each followed by a valid host-only call; with everything valid the call gets as far as the device.
    The device-resident calls refuse a null context.  (The refusals that need a context are in tests/test_gpu_strands.py.)
  - sa_dna_complement and sa_reverse_complement through the binding, against the reverse complement written in Python.
  - The tool: every refused combination of --strands, --help.
  - sa_host_write_search_strands of cli/libsa_host.so through ctypes: every dataset exact through h5dump, E = 0, each bad input an
    error that leaves the file as it was."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DUMP, ROOT, HostError, _Store
from tests.strands_cases import ALPHABET, COMPLEMENT, dna_database, dna_queries, rc
from tests.test_edges_host import h5_array
from tests.test_neighbors_host import h5_names
from tests.test_search_above_host import ListHost


# ---- the library ---------------------------------------------------------------------------------------------------------------
def still_answers(sa):
    """a valid call after a refusal: host-only, exact"""
    assert sa.norm_value(-7, 3, 5, sa.NORM_MIN) == (-7 * 1000000) // 3
    assert sa.dna_complement()[ord("R")] == ord("Y")


def test_complement_table_and_reverse_complement(sa):
    comp = sa.dna_complement()
    assert comp.dtype == np.uint8 and comp.shape == (128,)
    want = np.zeros(128, np.uint8)
    for a, b in COMPLEMENT.items():
        want[a] = b
    assert np.array_equal(comp, want)
    assert all(comp[comp[c]] == c for c in ALPHABET) and comp[ord("U")] == ord("A")  # an involution on its domain
    seqs = dna_database(40, seed=9, lo=1, hi=130) + [b"A", b"ACGT", bytes(ALPHABET)]
    store = sa.SequenceStore.from_sequences(seqs)
    once = sa.reverse_complement(store)
    assert [once.sequence(k) for k in range(store.num)] == [rc(s) for s in seqs]
    assert np.array_equal(once.meta, store.meta) and np.array_equal(once.blob == 0, store.blob == 0)  # the same meta, the same terminators
    assert sa.reverse_complement(once).blob.tobytes() == store.blob.tobytes()  # twice is the identity
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    assert sa.reverse_complement(store, scoring=scoring).blob.tobytes() == once.blob.tobytes()
    # refusals name the sequence (#1 is the first), the residue and the byte
    bad = sa.SequenceStore.from_sequences([b"ACGT", b"ACGT", b"ACGEAX"])
    with pytest.raises(sa.AlignError, match=r"sa_reverse_complement: sequence #3 has no reverse complement: residue 4 is byte 0x45 \('E'\), which has no complement"):
        sa.reverse_complement(bad)
    rna = sa.SequenceStore.from_sequences([b"ACGU"])
    assert sa.reverse_complement(rna).sequence(0) == b"ACGT"  # U -> A without a scoring ...
    mine = comp.copy()
    mine[ord("G")] = ord("U")  # ... and a table of the caller's whose complement nuc44 does not hold
    with pytest.raises(sa.AlignError, match=r"sequence #1 .* residue 3 is byte 0x47 \('G'\), whose complement 'U' the scoring's alphabet does not hold"):
        sa.reverse_complement(rna, comp=mine, scoring=scoring)
    with pytest.raises(sa.AlignError, match="a complement table is 128 uint8"):
        sa.reverse_complement(rna, comp=np.zeros(64, np.uint8))
    still_answers(sa)


def test_device_resident_calls_refuse_a_null_context(sa):
    lib = sa.load_library()
    for call, name in ((lambda: lib.sa_ctx_strand_fold(None, None, None, None, None, 1, None, None, None, None), "sa_ctx_strand_fold"),
                       (lambda: lib.sa_ctx_hits_strand(None, None, 1, 1, None, None, None), "sa_ctx_hits_strand"),
                       (lambda: lib.sa_ctx_hits_above_strand(None, None, 1, None, None, None, None), "sa_ctx_hits_above_strand")):
        assert call() != 0
        assert lib.sa_last_error().decode() == f"{name}: null context"
        still_answers(sa)
    assert lib.sa_ctx_search_strands(None) == 0 and lib.sa_hitlist_strand(None) is None
    assert sa.last_search_strands_seconds() >= 0.0


def test_the_one_call_forms_refuse_before_a_device_is_looked_for(sa):
    lib = sa.load_library()
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    db = sa.SequenceStore.from_sequences(dna_database(5, seed=3))
    queries = sa.SequenceStore.from_sequences(dna_queries(dna_database(5, seed=3), 3, seed=4))
    protein = sa.SequenceStore.from_sequences([b"ACGT", b"ACQT"])  # Q: no nucleotide
    empty = sa.SequenceStore.from_sequences([])
    sc = scoring._as_c()
    den = np.full(5 + 2 * 3, 77, np.int32)
    cn = sa.binding._Norm(sa.NORM_SELF, sa.NORM_MIN, den.ctypes.data)
    out = {name: np.full(3 * 5, 77, np.int32) for name in ("index", "value", "score", "rect", "vrect")}
    out8 = {name: np.full(3 * 5, 77, np.uint8) for name in ("strand", "srect")}
    order = ("index", "value", "score", "strand", "rect", "vrect", "srect")

    def topk(a=db, b=queries, s=C.byref(sc), k=2, norm=None, denom=None, want=order, comp=None):
        cd = None if denom is None else C.c_int32(denom)
        ptr = [({**out, **out8}[name].ctypes.data if name in want else None) for name in order]
        return lib.sa_hip_search_strands(a._as_c() if hasattr(a, "_as_c") else a, b._as_c() if hasattr(b, "_as_c") else b, s,
                                         None if comp is None else comp.ctypes.data, k, *ptr, None if norm is None else C.byref(norm),
                                         None if cd is None else C.byref(cd))

    def above(a=db, b=queries, s=C.byref(sc), norm=None, denom=None, comp=None, **_):
        cd = None if denom is None else C.c_int32(denom)
        return lib.sa_hip_search_above_strands(a._as_c() if hasattr(a, "_as_c") else a, b._as_c() if hasattr(b, "_as_c") else b, s,
                                               None if comp is None else comp.ctypes.data, 0, None if norm is None else C.byref(norm),
                                               None if cd is None else C.byref(cd))

    def reaches_the_device(call, **kw):
        if sa.device_count() == 0:
            assert not call(**kw) and b"No HIP devices" in lib.sa_last_error()

    def refused(message, calls=(topk, above), **kw):
        for call in calls:
            assert not call(**kw)
            text = lib.sa_last_error().decode()
            name = "sa_hip_search_strands: " if call is topk else "sa_hip_search_above_strands: "
            assert (text.startswith(name) or text.startswith("Query sequence")) and message in text, text
            still_answers(sa)
            reaches_the_device(call)

    refused("null argument", s=None)
    refused("norm and pid_denom exclude each other", norm=cn, denom=sa.PID_COLUMNS)
    refused("empty store", a=empty)
    refused("empty store", b=empty)
    refused("null sequence store", a=sa.binding._Input(None, None, 0, 5))
    refused("null sequence store", b=sa.binding._Input(None, None, 0, 3))
    for source, rule, message in ((2, 0, "source 2 is neither"), (0, 3, "rule 3 is none of")):
        refused(message, norm=sa.binding._Norm(source, rule, den.ctypes.data))
    for denom in (-1, 4):
        refused(f"denom {denom} is none of", denom=denom)
    refused("sequence #2 has no reverse complement: residue 3 is byte 0x51 ('Q'), which has no complement", b=protein)
    mine = sa.dna_complement()
    mine[ord("A")] = ord("U")
    refused("whose complement 'U' the scoring's alphabet does not hold", comp=mine)
    # the M x k outputs belong to index; k; nothing asked for
    refused("value, score and strand belong to the hits of index, which is null", calls=(topk,), want=("value",))
    refused("value, score and strand belong to the hits of index, which is null", calls=(topk,), want=("strand", "rect"))
    refused("nothing asked for", calls=(topk,), want=())
    refused("k = 0 hits", calls=(topk,), k=0)
    refused("k = 6 hits among 5 database sequences", calls=(topk,), k=6)
    assert (den == 77).all() and all((a == 77).all() for a in list(out.values()) + list(out8.values())), "a refused call wrote to its outputs"
    for kw in (dict(), dict(norm=cn), dict(denom=sa.PID_SHORTER), dict(want=("rect",), k=0), dict(want=("srect",)), dict(comp=sa.dna_complement())):
        reaches_the_device(topk, **kw)
        reaches_the_device(above, **kw)
    # the context itself refuses alike, before a device is looked for
    for message, b in (("sa_ctx_create_search_strands: sequence #2 has no reverse complement", protein), ("empty store", empty)):
        assert not lib.sa_ctx_create_search_strands(0, db._as_c(), b._as_c(), C.byref(sc), None)
        assert message in lib.sa_last_error().decode()
    assert not lib.sa_ctx_create_search_strands(0, db._as_c(), queries._as_c(), None, None) and b"null scoring" in lib.sa_last_error()


def test_binding_refusals(sa):
    scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
    db = sa.SequenceStore.from_sequences(dna_database(5, seed=3))
    queries = sa.SequenceStore.from_sequences([b"ACGT", b"ACCGT"])
    with pytest.raises(sa.AlignError, match="sa_hip_search_strands: norm and pid_denom exclude each other"):
        sa.hip_search_strands(db, queries, scoring, k=1, norm=sa.Norm(), pid=sa.PID_COLUMNS)
    with pytest.raises(sa.AlignError, match="nothing asked for"):
        sa.hip_search_strands(db, queries, scoring)
    with pytest.raises(sa.AlignError, match="min_value = 2147483648 is not an int32"):
        sa.hip_search_above_strands(db, queries, scoring, 2**31)
    with pytest.raises(sa.AlignError, match="sa_hip_search_above_strands: rule 5"):
        sa.hip_search_above_strands(db, queries, scoring, 0, norm=sa.Norm(sa.NORM_LENGTH, 5))
    assert sa.strand_words(1) == 1 and sa.strand_words(64) == 1 and sa.strand_words(65) == 2
    assert (sa.STRAND_FORWARD, sa.STRAND_REVERSE, sa.STRAND_NONE) == (0, 1, 255)
    still_answers(sa)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return exe


DNA = ["-a", "sw", "-m", "nuc44", "-s", "10", "-e", "1"]
REFUSED = [
    (DNA + ["--strands", "both"], "--strands both requires --query"),
    (DNA + ["--strands", "both", "-k", "2"], "--strands both requires --query"),
    (DNA + ["--strands", "both", "--hits-min", "5"], "--hits-min requires --query"),
    (["-a", "nw", "-m", "blosum62", "-p", "4", "--query", "Q", "-k", "2", "--strands", "both"], "--strands both and -m blosum62 conflict"),
    (["-a", "sw", "-m", "PAM250", "-s", "10", "-e", "1", "--query", "Q", "--hits-min", "5", "--strands", "both"], "--strands both and -m PAM250 conflict"),
    (DNA + ["--query", "Q", "-k", "2", "--strands", "reverse"], "Strands must be one of forward, both: reverse"),
    (DNA + ["--query", "Q", "-k", "2", "--strands", ""], "Strands must be one of forward, both: "),
    (DNA + ["--query", "Q", "--strands", "both"], "--query requires -k"),
    (DNA + ["--query", "Q", "-k", "2", "--strands", "both", "--min-score", "5"], "--query and --min-score conflict"),
    (DNA + ["--query", "Q", "-k", "2", "--strands", "both", "-z", "3"], "--query and -z, --compression conflict"),
]


@pytest.mark.parametrize("bad,message", REFUSED)
def test_refused_with_a_message_and_no_output(bad, message, cli, tmp_path):
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGACA\n>c\nGGGACGTRYA\n")
    queries.write_bytes(b">x\nACGTAC\n>y\nTTGACA\n")
    bad = [str(queries) if word == "Q" else word for word in bad]
    res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-F", "-P", *bad], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and message in res.stderr and "usage information" in res.stderr, res.stdout + res.stderr
    assert not out.exists()


def test_a_query_residue_without_a_complement_ends_the_run(cli, tmp_path):
    """the alphabet of the shipped nucleotide tables IS the complement table's domain, so the loader is what refuses such a query (U, or
    an amino-acid letter); the tool's own check behind it says what sa_reverse_complement says (test_complement_table_... above)"""
    fasta, out = tmp_path / "in.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGACA\n")
    for residue in (b"U", b"E", b"Q"):
        queries = tmp_path / "q.fasta"
        queries.write_bytes(b">x\nACGTAC\n>y\nTTG" + residue + b"ACA\n")
        res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-F", "-P", *DNA, "--query", str(queries), "-k", "1", "--strands", "both"],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and "Sequence #2 is invalid" in res.stderr and "No HIP devices" not in res.stderr, res.stdout + res.stderr
        assert not out.exists()


@pytest.mark.parametrize("extra", [["-k", "2"], ["-k", "2", "--alignments", "--query-scores"], ["-k", "1", "--hits-by", "identity-shorter"],
                                   ["--hits-min", "5"], ["--hits-min", "5", "--hits-by", "len-min", "--query-scores"]])
def test_accepted_options_get_as_far_as_the_device(extra, cli, tmp_path, sa):
    if sa.device_count() != 0:
        return  # (a device is present: tests/test_gpu_strands_cli.py runs these to the end)
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGACA\n>c\nGGGACGTRYA\n")
    queries.write_bytes(b">x\nACGTAC\n>y\nTTGNACA\n")
    for strands in ("both", "forward"):
        res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-F", "-P", *DNA, "--query", str(queries), "--strands", strands, *extra],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and "No HIP devices" in res.stderr and "usage information" not in res.stderr, res.stdout + res.stderr
        assert ("Strands: both" in res.stdout) == (strands == "both")
        assert not out.exists()


def test_help_documents_the_option(cli):
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--strands WHICH", "forward (the default", "both:", "/hit_strands", "/hitlist_strands", "/query_strands", "REVERSE COMPLEMENT",
                 "length - 1 - p", "the forward one on", "nucleotide matrix"):
        assert word in text, word


# ---- the writer ----------------------------------------------------------------------------------------------------------------
class StrandsHost(ListHost):
    """the suite's host binding plus sa_host_write_search and the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_search.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_int32] + [C.c_void_p] * 5 + [C.c_int64]
        self.lib.sa_host_write_search.restype = C.c_int
        self.lib.sa_host_write_search_strands.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_int32, C.c_void_p, C.c_int64,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.sa_host_write_search_strands.restype = C.c_int

    def stores(self, db, queries, lut):
        return (self.parse(b"".join(b">s\n" + s + b"\n" for s in db), "fasta", lut), self.parse(b"".join(b">s\n" + s + b"\n" for s in queries), "fasta", lut))

    def write_search(self, path, db, queries, lut, k, index, score):
        sd, sq = self.stores(db, queries, lut)
        try:
            i, s = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(score, np.int32)
            if self.lib.sa_host_write_search(str(path).encode(), C.byref(sd), C.byref(sq), k, i.ctypes.data, s.ctypes.data, None, None, None, 0):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(sd))
            self.lib.sa_host_store_free(C.byref(sq))

    def write_strands(self, path, db, queries, lut, k=0, hit=None, count=-1, listed=None, rect=None, den=None):
        sd, sq = self.stores(db, queries, lut)
        try:
            keep = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (hit, listed, rect)]
            d = None if den is None else np.ascontiguousarray(den, np.int32)
            ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
            if self.lib.sa_host_write_search_strands(str(path).encode(), C.byref(sd), C.byref(sq), k, ptr(keep[0]), count, ptr(keep[1]), ptr(keep[2]),
                                                     ptr(d)):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(sd))
            self.lib.sa_host_store_free(C.byref(sq))


@pytest.fixture(scope="module")
def host():
    return StrandsHost()


@pytest.fixture(scope="module")
def dna_lut(sa):
    return sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1).lut


def topk_file(host, lut, path, n, m, k, seed):
    rng = np.random.default_rng(seed)
    db = dna_database(n, seed=seed, lo=8, hi=30)
    queries = dna_database(m, seed=seed + 1, lo=8, hi=30)
    index = np.stack([rng.permutation(n)[:k] for _ in range(m)]).astype(np.int32)
    score = rng.integers(-1000, 1000, (m, k)).astype(np.int32)
    host.write_search(path, db, queries, lut, k, index, score)
    return db, queries, rng


def test_strands_of_a_top_k_file(host, dna_lut, tmp_path):
    n, m, k = 40, 7, 5
    path = tmp_path / "s.h5"
    db, queries, rng = topk_file(host, dna_lut, path, n, m, k, 5)
    before = h5_names(path)
    hit, rect = rng.integers(0, 2, (m, k)).astype(np.uint8), rng.integers(0, 2, (m, n)).astype(np.uint8)
    den = rng.integers(1, 4000, m).astype(np.int32)
    host.write_strands(path, db, queries, dna_lut, k=k, hit=hit, rect=rect, den=den)
    assert h5_names(path) == before | {"/hit_strands", "/query_strands", "/query_reverse_denominators"}
    assert np.array_equal(h5_array(path, "hit_strands", "u1").reshape(m, k), hit)
    assert np.array_equal(h5_array(path, "query_strands", "u1").reshape(m, n), rect)
    assert np.array_equal(h5_array(path, "query_reverse_denominators", "<i4"), den)
    txt = subprocess.run([str(H5DUMP), "-H", "-d", "/hit_strands", str(path)], capture_output=True, text=True, check=True).stdout
    assert "H5T_STD_U8LE" in txt and f"( {m}, {k} )" in txt, txt
    # the hits alone
    path = tmp_path / "t.h5"
    db, queries, rng = topk_file(host, dna_lut, path, n, m, k, 6)
    host.write_strands(path, db, queries, dna_lut, k=k, hit=hit)
    assert h5_names(path) == before | {"/hit_strands"}


def test_strands_of_a_hit_list_file(host, dna_lut, tmp_path):
    n, m = 30, 4
    rng = np.random.default_rng(8)
    db, queries = dna_database(n, seed=8, lo=8, hi=30), dna_database(m, seed=9, lo=8, hi=30)
    counts = np.array([0, n, 3, 7])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    index = np.concatenate([np.sort(rng.permutation(n)[:c]) for c in counts]).astype(np.int32)
    e = int(offsets[-1])
    score = rng.integers(-1000, 1000, e).astype(np.int32)
    path = tmp_path / "l.h5"
    host.write_list(path, db, queries, dna_lut, offsets, index, score, 17)
    before = h5_names(path)
    listed, rect = rng.integers(0, 2, e).astype(np.uint8), rng.integers(0, 2, (m, n)).astype(np.uint8)
    host.write_strands(path, db, queries, dna_lut, count=e, listed=listed, rect=rect)
    assert h5_names(path) == before | {"/hitlist_strands", "/query_strands"}
    assert np.array_equal(h5_array(path, "hitlist_strands", "u1"), listed)
    assert np.array_equal(h5_array(path, "query_strands", "u1").reshape(m, n), rect)
    # E = 0: the dataset is there with extent 0; the array may be NULL
    path = tmp_path / "none.h5"
    host.write_list(path, db, queries, dna_lut, np.zeros(m + 1, np.int64), None, None, 2**31 - 1)
    host.write_strands(path, db, queries, dna_lut, count=0, listed=None)
    assert h5_names(path) == before | {"/hitlist_strands"} and h5_array(path, "hitlist_strands", "u1").size == 0


def test_bad_inputs_are_errors_and_leave_the_file_as_it_was(host, dna_lut, tmp_path):
    n, m, k = 20, 3, 4
    path = tmp_path / "s.h5"
    db, queries, rng = topk_file(host, dna_lut, path, n, m, k, 11)
    before = h5_names(path)
    hit, rect = rng.integers(0, 2, (m, k)).astype(np.uint8), rng.integers(0, 2, (m, n)).astype(np.uint8)
    two, rect_two = hit.copy(), rect.copy()
    two[1, 2], rect_two[2, 7] = 2, 255
    bad = [("Strand data missing", dict(k=k, hit=None)),
           ("Strand 2 of hit 6 is neither forward", dict(k=k, hit=two)),
           ("Strand 255 of query 2 against database sequence 7 is neither forward", dict(k=k, hit=hit, rect=rect_two)),
           ("Hit count must be between 1 and 64", dict(k=0, hit=hit)),
           ("Hit count must be between 1 and 64", dict(k=65, hit=hit)),
           ("Hit count must be between 1 and 64", dict(k=n + 1, hit=hit)),
           ("The strands of a hit list go without a hit count", dict(k=k, count=3, listed=hit)),
           ("Strand data missing", dict(count=3, listed=None)),
           (r"holds no /hit_indices of 3 x 3 hits", dict(k=3, hit=hit[:, :3])),
           (r"holds no /hitlist_indices of 5 hits", dict(count=5, listed=np.zeros(5, np.uint8)))]
    for message, kw in bad:
        with pytest.raises(HostError, match=message):
            host.write_strands(path, db, queries, dna_lut, **kw)
        assert h5_names(path) == before, message
    with pytest.raises(HostError, match="Failed to open HDF5 file"):
        host.write_strands(tmp_path / "absent.h5", db, queries, dna_lut, k=k, hit=hit)
    assert not (tmp_path / "absent.h5").exists()
    host.write_strands(path, db, queries, dna_lut, k=k, hit=hit)
    with pytest.raises(HostError, match="already holds /hit_strands"):
        host.write_strands(path, db, queries, dna_lut, k=k, hit=hit)
    assert np.array_equal(h5_array(path, "hit_strands", "u1").reshape(m, k), hit)
