"""CPU: what the fitted search (csrc/sa_fit.hip, --fit) needs no device for.
  - Every refusal of sa_hip_search_fit that comes before a device is looked for, with its message, each followed by a valid host-only
    call; with everything valid the call gets as far as the device.  The device-resident calls refuse a null context.  (The refusals
    that need a context -- an ordinary one, SW, the outputs, the queries -- are in tests/test_gpu_fit.py.)
  - The tool: every refused combination of --fit, --help, the accepted ones as far as the device.
  - sa_host_write_search_fit of cli/libsa_host.so through ctypes: every dataset exact through h5dump, each bad input an error that
    leaves the file as it was."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DUMP, ROOT, HostError, _Store
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_neighbors_host import h5_names
from tests.test_search_above_host import ListHost


def still_answers(sa):
    """a valid call after a refusal: host-only, exact"""
    assert sa.norm_value(-7, 3, 5, sa.NORM_MIN) == (-7 * 1000000) // 3
    assert sa.pid_value(3, 7, 5, 9, sa.PID_COLUMNS) == 3000000 // 7


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_device_resident_calls_refuse_a_null_context(sa):
    lib = sa.load_library()
    out = sa.binding._FitOut(None, None, None, None, None, None, 0)
    assert lib.sa_ctx_fit_rect(None, 0, 1, C.byref(out), None) != 0 and lib.sa_last_error().decode() == "sa_ctx_fit_rect: null context"
    still_answers(sa)
    assert lib.sa_ctx_fit_pairs(None, None, None, 1, C.byref(out), None) != 0 and lib.sa_last_error().decode() == "sa_ctx_fit_pairs: null context"
    still_answers(sa)
    assert lib.sa_ctx_fit_alignments(None, None, None, 0) is None and lib.sa_last_error().decode() == "sa_ctx_fit_alignments: null context"
    still_answers(sa)
    assert sa.last_search_fit_seconds() >= 0.0


def test_the_one_call_refuses_before_a_device_is_looked_for(sa):
    lib = sa.load_library()
    nw = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    sw = sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1)
    db = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    queries = sa.SequenceStore.from_sequences(make_protein_set(3, 4, 9, 4))
    empty = sa.SequenceStore.from_sequences([])
    order = ("index", "value", "score", "db_begin", "db_end", "rect", "vrect")
    out = {name: np.full(3 * 5, 77, np.int32) for name in order}
    c_nw, c_sw = nw._as_c(), sw._as_c()

    def call(a=db, b=queries, s=C.byref(c_nw), k=2, denom=-1, want=order):
        ptr = [(out[name].ctypes.data if name in want else None) for name in order]
        return lib.sa_hip_search_fit(a._as_c() if hasattr(a, "_as_c") else a, b._as_c() if hasattr(b, "_as_c") else b, s, k, denom, *ptr)

    def refused(message, **kw):
        assert not call(**kw)
        text = lib.sa_last_error().decode()
        assert text.startswith("sa_hip_search_fit: ") and message in text, text
        still_answers(sa)

    refused("null argument", s=None)
    refused("SW is local already; fit is defined for NW and Gotoh", s=C.byref(c_sw))
    refused("empty store", a=empty)
    refused("empty store", b=empty)
    refused("null sequence store", a=sa.binding._Input(None, None, 0, 5))
    refused("null sequence store", b=sa.binding._Input(None, None, 0, 3))
    for denom in (-2, 4, 2 ** 31 - 1):
        refused(f"denom {denom} is none of", denom=denom)
    refused("value, score, db_begin and db_end belong to the hits of index, which is null", want=("value",))
    refused("value, score, db_begin and db_end belong to the hits of index, which is null", want=("db_begin", "db_end", "rect"))
    refused("nothing asked for", want=())
    refused("k = 0 hits", k=0)
    refused("k = 6 hits among 5 database sequences", k=6)
    refused("k = 65 hits", k=65)
    assert all((a == 77).all() for a in out.values()), "a refused call wrote to its outputs"
    if sa.device_count() == 0:  # with everything valid the call gets as far as the device
        for kw in (dict(), dict(denom=sa.PID_SHORTER), dict(want=("rect",), k=0), dict(want=("index", "db_begin"))):
            assert not call(**kw) and b"No HIP devices" in lib.sa_last_error()
    with pytest.raises(sa.AlignError, match="nothing asked for"):
        sa.hip_search_fit(db, queries, nw)
    with pytest.raises(sa.AlignError, match="sa_hip_search_fit: method 2: SW is local already"):
        sa.hip_search_fit(db, queries, sw, k=1)
    with pytest.raises(sa.AlignError, match="denom = 4294967296 is not an int32"):
        sa.hip_search_fit(db, queries, nw, k=1, pid=2 ** 32)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return exe


NW = ["-a", "nw", "-m", "blosum62", "-p", "4"]
REFUSED = [
    (NW + ["--fit"], "--fit requires --query"),
    (NW + ["--fit", "-k", "2"], "--fit requires --query"),
    (["-a", "sw", "-m", "blosum62", "-s", "10", "-e", "1", "--query", "Q", "-k", "2", "--fit"], "--fit and -a sw conflict"),
    (NW + ["--query", "Q", "--hits-min", "5", "--fit"], "--fit and --hits-min conflict"),
    (["-a", "nw", "-m", "nuc44", "-p", "4", "--query", "Q", "-k", "2", "--strands", "both", "--fit"], "--fit and --strands both conflict"),
    (NW + ["--query", "Q", "-k", "2", "--fit", "--hits-by", "self-min"], "--fit and --hits-by self-min conflict"),
    (NW + ["--query", "Q", "-k", "2", "--fit", "--hits-by", "len-mean"], "--fit and --hits-by len-mean conflict"),
    (NW + ["--query", "Q", "--fit"], "--query requires -k"),
    (NW + ["--query", "Q", "-k", "2", "--fit", "--min-score", "5"], "--query and --min-score conflict"),
]


@pytest.mark.parametrize("bad,message", REFUSED)
def test_refused_with_a_message_and_no_output(bad, message, cli, tmp_path):
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGACA\n>c\nGGGACGTACA\n")
    queries.write_bytes(b">x\nACGTAC\n>y\nTTGACA\n")
    bad = [str(queries) if word == "Q" else word for word in bad]
    res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-F", "-P", *bad], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and message in res.stderr and "usage information" in res.stderr, res.stdout + res.stderr
    assert not out.exists()


@pytest.mark.parametrize("extra", [["-k", "2"], ["-k", "2", "--alignments", "--query-scores"], ["-k", "1", "--hits-by", "identity-columns"],
                                   ["-k", "3", "--hits-by", "score"]])
def test_accepted_options_get_as_far_as_the_device(extra, cli, tmp_path, sa):
    if sa.device_count() != 0:
        return  # (a device is present: tests/test_gpu_fit_cli.py runs these to the end)
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGACA\n>c\nGGGACGTACA\n")
    queries.write_bytes(b">x\nACGTAC\n>y\nTTGACA\n")
    for method in (NW, ["-a", "ga", "-m", "blosum62", "-s", "10", "-e", "1"]):
        res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-F", "-P", *method, "--query", str(queries), "--fit", *extra],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and "No HIP devices" in res.stderr and "usage information" not in res.stderr, res.stdout + res.stderr
        assert "Fit: every query whole" in res.stdout
        assert not out.exists()


def test_help_documents_the_option(cli):
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--fit ", "INSIDE the database sequence", "/hit_db_begin and /hit_db_end", "/search_ends", "-a sw (local already)", "--hits-min, --strands both"):
        assert word in text, word


# ---- the writer ----------------------------------------------------------------------------------------------------------------
class FitHost(ListHost):
    """the suite's host binding plus sa_host_write_search and the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_search.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_int32] + [C.c_void_p] * 5 + [C.c_int64]
        self.lib.sa_host_write_search.restype = C.c_int
        self.lib.sa_host_write_search_fit.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.sa_host_write_search_fit.restype = C.c_int

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

    def write_fit(self, path, db, queries, lut, k, index, begin, end):
        sd, sq = self.stores(db, queries, lut)
        try:
            keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (index, begin, end)]
            if self.lib.sa_host_write_search_fit(str(path).encode(), C.byref(sd), C.byref(sq), k, *[None if a is None else a.ctypes.data for a in keep]):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(sd))
            self.lib.sa_host_store_free(C.byref(sq))


@pytest.fixture(scope="module")
def host():
    return FitHost()


@pytest.fixture(scope="module")
def lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def search_file(host, lut, path, n, m, k, seed):
    rng = np.random.default_rng(seed)
    db, queries = make_protein_set(n, 8, 30, seed), make_protein_set(m, 3, 12, seed + 1)
    index = np.stack([rng.permutation(n)[:k] for _ in range(m)]).astype(np.int32)
    score = rng.integers(-1000, 1000, (m, k)).astype(np.int32)
    host.write_search(path, db, queries, lut, k, index, score)
    lens = np.array([len(s) for s in db])[index]
    begin = (rng.integers(0, 1000, (m, k)) % (lens + 1)).astype(np.int32)
    end = (begin + rng.integers(0, 1000, (m, k)) % (lens - begin + 1)).astype(np.int32)
    begin[0, 0], end[0, 0] = 0, 0          # the query against nothing
    begin[1, 1], end[1, 1] = 0, lens[1, 1]  # the whole database sequence
    return db, queries, index, begin, end, lens


def test_spans_of_a_search_file(host, lut, tmp_path):
    n, m, k = 30, 6, 4
    path = tmp_path / "s.h5"
    db, queries, index, begin, end, lens = search_file(host, lut, path, n, m, k, 5)
    before = h5_names(path)
    host.write_fit(path, db, queries, lut, k, index, begin, end)
    assert h5_names(path) == before | {"/hit_db_begin", "/hit_db_end", "/search_ends"}
    assert np.array_equal(h5_array(path, "hit_db_begin", "<i4").reshape(m, k), begin)
    assert np.array_equal(h5_array(path, "hit_db_end", "<i4").reshape(m, k), end)
    assert h5_array(path, "search_ends", "<i4").tolist() == [1]
    assert np.array_equal(h5_array(path, "hit_indices", "<i4").reshape(m, k), index)  # the other datasets stay
    txt = subprocess.run([str(H5DUMP), "-H", "-d", "/hit_db_end", str(path)], capture_output=True, text=True, check=True).stdout
    assert "H5T_STD_I32LE" in txt and f"( {m}, {k} )" in txt, txt


def test_bad_inputs_are_errors_and_leave_the_file_as_it_was(host, lut, tmp_path):
    n, m, k = 20, 3, 4
    path = tmp_path / "s.h5"
    db, queries, index, begin, end, lens = search_file(host, lut, path, n, m, k, 11)
    before = h5_names(path)

    def changed(a, at, v):
        b = a.copy()
        b[at] = v
        return b

    bad = [("Fit data missing", dict(k=k, index=index, begin=None, end=end)),
           ("Fit data missing", dict(k=k, index=None, begin=begin, end=end)),
           (r"Span \[-1, .*\) of hit 2 of query 1 is outside", dict(k=k, index=index, begin=changed(begin, (1, 2), -1), end=end)),
           (rf"Span \[.*, {lens[2, 3] + 1}\) of hit 3 of query 2 is outside its database sequence of {lens[2, 3]} residues",
            dict(k=k, index=index, begin=begin, end=changed(end, (2, 3), lens[2, 3] + 1))),
           (r"Span \[5, 4\) of hit 0 of query 2 is outside", dict(k=k, index=index, begin=changed(begin, (2, 0), 5), end=changed(end, (2, 0), 4))),
           ("Hit index 20 of query 0 outside the 20 database sequences", dict(k=k, index=changed(index, (0, 1), 20), begin=begin, end=end)),
           ("Hit count must be between 1 and 64", dict(k=0, index=index, begin=begin, end=end)),
           ("Hit count must be between 1 and 64", dict(k=65, index=index, begin=begin, end=end)),
           (r"holds no /hit_indices of 3 x 3 hits", dict(k=3, index=index[:, :3], begin=begin[:, :3], end=end[:, :3]))]
    for message, kw in bad:
        with pytest.raises(HostError, match=message):
            host.write_fit(path, db, queries, lut, **kw)
        assert h5_names(path) == before, message
    with pytest.raises(HostError, match="Failed to open HDF5 file"):
        host.write_fit(tmp_path / "absent.h5", db, queries, lut, k, index, begin, end)
    assert not (tmp_path / "absent.h5").exists()
    host.write_fit(path, db, queries, lut, k, index, begin, end)
    with pytest.raises(HostError, match="already holds /hit_db_begin"):
        host.write_fit(path, db, queries, lut, k, index, begin, end)
    assert np.array_equal(h5_array(path, "hit_db_begin", "<i4").reshape(m, k), begin)
