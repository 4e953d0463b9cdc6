"""CPU: what the search quantities (csrc/sa_search_quantity.hip, --hits-by) need no device for.
  - Every refusal of sa_ctx_normalize_rect, sa_ctx_identity_rect, sa_ctx_hits_take, sa_hip_search_norm and sa_hip_search_pid that
    comes before a device is looked for, with its message, each followed by a valid host-only call: the refusal leaves no state
    behind.  (The refusals that need a context are in tests/test_gpu_search_quantity.py.)
  - The tool: --hits-by without --query, an unknown quantity, --help; the refusals tests/test_search_cli_host.py pins still hold
    beside the new option.
  - sa_host_write_search_values of cli/libsa_host.so through ctypes: the datasets it adds are exact, the ones that were there
    keep their bytes, a file it cannot finish is left as it was."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.host_binding import ROOT, HostError, _Store
from tests.search_cases import h5_strings
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_neighbors_host import h5_names
from tests.test_search_cli_host import SearchHost, case

QUANTITIES = ("score", "self-min", "self-max", "self-mean", "len-min", "len-max", "len-mean", "identity-columns", "identity-shorter",
              "identity-longer", "identity-mean")


# ---- the library ---------------------------------------------------------------------------------------------------------------
def still_answers(sa):
    """a valid call after a refusal: the value rules on the host, exact"""
    assert sa.norm_value(-7, 3, 5, sa.NORM_MIN) == (-7 * 1000000) // 3
    assert sa.pid_value(3, 7, 10, 12, sa.PID_COLUMNS) == 3 * 1000000 // 7


def test_context_calls_refuse_a_null_context(sa):
    lib = sa.load_library()
    out = sa.binding._IdentityOut(None, None, None, None, 0)
    for call, name in ((lambda: lib.sa_ctx_normalize_rect(None, None, 1, 0, None, 0, None, None), "sa_ctx_normalize_rect"),
                       (lambda: lib.sa_ctx_identity_rect(None, 0, 1, C.byref(out), None), "sa_ctx_identity_rect"),
                       (lambda: lib.sa_ctx_hits_take(None, None, 1, 1, None, None, None), "sa_ctx_hits_take")):
        assert call() != 0
        assert lib.sa_last_error().decode() == f"{name}: null context"
        still_answers(sa)


@pytest.mark.parametrize("which", ["norm", "pid"])
def test_one_call_forms_refuse_before_a_device_is_looked_for(which, sa):
    lib = sa.load_library()
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    db = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    queries = sa.SequenceStore.from_sequences(make_protein_set(3, 8, 12, 4))
    empty = sa.SequenceStore.from_sequences([])
    who = f"sa_hip_search_{which}"
    sc = scoring._as_c()
    den = np.full(8, 77, np.int32)
    cn = sa.binding._Norm(sa.NORM_SELF, sa.NORM_MIN, den.ctypes.data)
    bufs = [np.full(15, 77, np.int32) for _ in range(5)]
    index, value, score, rect, vrect = (b.ctypes.data for b in bufs)

    def call(a=db, b=queries, s=C.byref(sc), k=3, out=(index, value, score, rect, vrect), norm=cn, denom=sa.PID_COLUMNS):
        if which == "norm":
            return lib.sa_hip_search_norm(a._as_c() if hasattr(a, "_as_c") else a, b._as_c() if hasattr(b, "_as_c") else b, s, k, *out,
                                          None if norm is None else C.byref(norm))
        return lib.sa_hip_search_pid(a._as_c() if hasattr(a, "_as_c") else a, b._as_c() if hasattr(b, "_as_c") else b, s, k, *out, denom)

    def refused(message, **kw):
        assert not call(**kw)
        assert lib.sa_last_error().decode().startswith(who + ": ") and message in lib.sa_last_error().decode(), lib.sa_last_error()
        still_answers(sa)

    refused("null argument", s=None)
    refused("value and score belong to the hits of index", out=(None, value, None, None, None))
    refused("value and score belong to the hits of index", out=(None, None, score, rect, None))
    refused("nothing asked for", out=(None, None, None, None, None))
    refused("empty store", a=empty)
    refused("empty store", b=empty)
    refused("null sequence store", a=sa.binding._Input(None, None, 0, 5))
    for k in (0, -1, 6, 65, 2 ** 31 - 1):
        refused("k must be in [1, min(N, 64)]", k=k)
    if which == "norm":
        for source, rule, message in ((2, 0, "source 2 is neither"), (-1, 0, "source -1 is neither"), (0, 3, "rule 3 is none of"), (0, -1, "rule -1 is none of")):
            refused(message, norm=sa.binding._Norm(source, rule, den.ctypes.data))
        # norm == NULL is sa_hip_search: its own argument checks, under this call's name where they come first
        refused("nothing asked for", norm=None, out=(None, None, None, None, None))
        refused("k must be in [1, min(N, 64)]", norm=None, k=6)
    else:
        for denom in (-1, 4, 2 ** 31 - 1):
            refused(f"denom {denom} is none of", denom=denom)
    assert all((b == 77).all() for b in bufs) and (den == 77).all(), "a refused call wrote to its outputs"
    # ... and with everything valid the call gets as far as the device
    if sa.device_count() == 0:
        assert not call() and b"No HIP devices" in lib.sa_last_error()


def test_binding_refusals(sa):
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    db = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    queries = sa.SequenceStore.from_sequences(make_protein_set(3, 8, 12, 4))
    with pytest.raises(ValueError, match="exclude each other"):
        sa.hip_search(db, queries, scoring, k=2, norm=sa.Norm(), pid=sa.PID_COLUMNS)
    with pytest.raises(sa.AlignError, match="nothing asked for"):
        sa.hip_search(db, queries, scoring, norm=sa.Norm())
    with pytest.raises(sa.AlignError, match=r"sa_hip_search_pid: k = 6 hits"):
        sa.hip_search(db, queries, scoring, k=6, pid=sa.PID_MEAN)
    with pytest.raises(sa.AlignError, match=r"sa_hip_search_norm: rule 5"):
        sa.hip_search(db, queries, scoring, k=2, norm=sa.Norm(sa.NORM_LENGTH, 5))
    assert sa.last_search_quantity_seconds() >= 0.0
    still_answers(sa)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return exe


REFUSED = [
    (["--hits-by", "self-min"], "--hits-by requires --query"),
    (["--hits-by", "score"], "--hits-by requires --query"),
    (["--hits-by", "self-min", "-k", "2"], "--hits-by requires --query"),
    (["--query", "Q", "-k", "2", "--hits-by", "self"], "Hit quantity must be one of score, self-min"),
    (["--query", "Q", "-k", "2", "--hits-by", "identity"], "Hit quantity must be one of score, self-min"),
    (["--query", "Q", "-k", "2", "--hits-by", "columns"], "Hit quantity must be one of score, self-min"),
    # what tests/test_search_cli_host.py pins, beside the new option as well
    (["--query", "Q", "-k", "2", "--normalize", "self-min"], "--query and --normalize conflict"),
    (["--query", "Q", "-k", "2", "--identity", "columns"], "--query and --identity conflict"),
    (["--query", "Q", "-k", "2", "--hits-by", "self-min", "--normalize", "self-min"], "--query and --normalize conflict"),
    (["--query", "Q", "-k", "2", "--hits-by", "identity-columns", "--identity", "columns"], "--query and --identity conflict"),
    (["--query", "Q", "-k", "2", "--hits-by", "len-max", "--linkage"], "--query and --linkage conflict"),
    (["--query", "Q", "--hits-by", "len-max"], "--query requires -k"),
    (["--query", "Q", "-k", "4", "--hits-by", "len-max"], "Hit count 4 exceeds the 3 database sequences"),
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


def test_help_documents_the_option(cli):
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--hits-by QUANTITY", *QUANTITIES, "/hit_values", "/hit_quantity", "/hit_scale", "/database_denominators", "/query_denominators",
                 "/query_values", "NO LONGER", "SORTED"):
        assert word in text, word


# ---- the writer ----------------------------------------------------------------------------------------------------------------
class ValuesHost(SearchHost):
    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_search_values.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_int32, C.c_void_p, C.c_int32,
                                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        self.lib.sa_host_write_search_values.restype = C.c_int

    def write_values(self, path, db, queries, lut, k, value, kind, source, rule, den=None, vrect=None):
        sd = self.parse(b"".join(b">s\n" + s + b"\n" for s in db), "fasta", lut)
        sq = self.parse(b"".join(b">s\n" + s + b"\n" for s in queries), "fasta", lut)
        try:
            value = np.ascontiguousarray(value, np.int32)
            den = None if den is None else np.ascontiguousarray(den, np.int32)
            vrect = None if vrect is None else np.ascontiguousarray(vrect, np.int32)
            if self.lib.sa_host_write_search_values(str(path).encode(), C.byref(sd), C.byref(sq), int(k), value.ctypes.data, kind, source, rule,
                                                    None if den is None else den.ctypes.data, None if vrect is None else vrect.ctypes.data):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(sd))
            self.lib.sa_host_store_free(C.byref(sq))


@pytest.fixture(scope="module")
def host():
    return ValuesHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


EARLIER = (("hit_indices", "<i4"), ("hit_scores", "<i4"), ("query_scores", "<i4"), ("hit_alignment_records", "<i4"), ("hit_cigar_offsets", "<i8"),
           ("hit_cigars", "<u4"))


def values_case(n, m, k, seed):
    rng = np.random.default_rng(seed)
    value = -np.sort(-rng.integers(-2 ** 31, 2 ** 31 - 1, (m, k), dtype=np.int64), axis=1).astype(np.int32)
    den = rng.integers(-5, 4000, n + m).astype(np.int32)
    vrect = rng.integers(-2 ** 31, 2 ** 31 - 1, (m, n), dtype=np.int64).astype(np.int32)
    return value, den, vrect


def earlier(path):
    return {name: h5_array(path, name, dtype).tobytes() for name, dtype in EARLIER}


@pytest.mark.parametrize("kind,source,rule", [(1, 0, 0), (1, 1, 2), (2, 0, 3)])
def test_values_are_added_and_the_rest_keeps_its_bytes(kind, source, rule, host, protein_lut, tmp_path):
    n, m, k = 40, 7, 3
    db, queries, index, score, rect, records, cigar = case(n, m, k, 6)
    value, den, vrect = values_case(n, m, k, 16)
    path = tmp_path / "s.h5"
    host.write_search(path, db, queries, protein_lut, k, index, score, rect, records, cigar)
    names, before = h5_names(path), earlier(path)
    host.write_values(path, db, queries, protein_lut, k, value, kind, source, rule, den if kind == 1 else None, vrect)
    added = {"/hit_values", "/hit_quantity", "/hit_scale", "/query_values"} | ({"/database_denominators", "/query_denominators"} if kind == 1 else set())
    assert h5_names(path) == names | added
    assert earlier(path) == before
    assert h5_strings(path, "sequences") == db and h5_strings(path, "query_sequences") == queries
    assert np.array_equal(h5_array(path, "hit_values", "<i4").reshape(m, k), value)
    assert h5_array(path, "hit_quantity", "<i4").tolist() == [kind, source if kind == 1 else 0, rule]
    assert h5_array(path, "hit_scale", "<i4").tolist() == [1000000]
    assert np.array_equal(h5_array(path, "query_values", "<i4").reshape(m, n), vrect)
    if kind == 1:
        assert np.array_equal(h5_array(path, "database_denominators", "<i4"), den[:n])
        assert np.array_equal(h5_array(path, "query_denominators", "<i4"), den[n:])


def test_values_alone(host, protein_lut, tmp_path):
    n, m, k = 300, 20, 64
    db, queries, index, score, _, _, _ = case(n, m, k, 5)
    value, _, _ = values_case(n, m, k, 15)
    path = tmp_path / "s.h5"
    host.write_search(path, db, queries, protein_lut, k, index, score)
    host.write_values(path, db, queries, protein_lut, k, value, 2, 0, 1)
    assert h5_names(path) == {"/sequences", "/query_sequences", "/hit_indices", "/hit_scores", "/hit_values", "/hit_quantity", "/hit_scale"}
    assert np.array_equal(h5_array(path, "hit_values", "<i4").reshape(m, k), value)
    assert h5_array(path, "hit_quantity", "<i4").tolist() == [2, 0, 1]


def test_a_file_that_cannot_be_finished_is_left_as_it_was(host, protein_lut, tmp_path):
    n, m, k = 40, 7, 3
    db, queries, index, score, rect, _, _ = case(n, m, k, 7)
    value, den, vrect = values_case(n, m, k, 17)
    path = tmp_path / "s.h5"
    host.write_search(path, db, queries, protein_lut, k, index, score, rect)
    image = path.read_bytes()
    unsorted = value.copy()
    unsorted[3] = unsorted[3, ::-1]
    assert unsorted[3, 0] < unsorted[3, -1]
    for message, kw in (("Hit count must be between 1 and 64", dict(k=0)),
                        ("Hit count must be between 1 and 64", dict(k=65)),
                        ("neither normalised score (1) nor percent identity (2)", dict(kind=0)),
                        ("Normalization source 2", dict(source=2)),
                        ("Normalization rule 3", dict(rule=3)),
                        ("Identity denominator 4", dict(kind=2, rule=4)),
                        ("Hit value data missing", dict(den=None)),
                        ("not in descending order", dict(value=unsorted)),
                        ("holds no /hit_indices of 7 x 2 hits", dict(k=2, value=value[:, :2])),
                        ("holds no /hit_indices of 6 x 3 hits", dict(queries=queries[:6], value=value[:6]))):
        args = dict(db=db, queries=queries, k=k, value=value, kind=1, source=0, rule=0, den=den, vrect=vrect)
        args.update(kw)
        with pytest.raises(HostError, match=message.replace("(", r"\(").replace(")", r"\)")):
            host.write_values(path, args["db"], args["queries"], protein_lut, args["k"], args["value"], args["kind"], args["source"], args["rule"],
                              args["den"], args["vrect"])
        assert path.read_bytes() == image, message
    # a file that is no search's, and no file at all
    plain = tmp_path / "plain.h5"
    host.write_hdf5(plain, db, protein_lut, np.zeros(n * (n - 1) // 2, np.int32), True)
    image_plain = plain.read_bytes()
    with pytest.raises(HostError, match="holds no /hit_indices"):
        host.write_values(plain, db, queries, protein_lut, k, value, 1, 0, 0, den)
    assert plain.read_bytes() == image_plain
    with pytest.raises(HostError, match="Failed to open HDF5 file"):
        host.write_values(tmp_path / "missing.h5", db, queries, protein_lut, k, value, 1, 0, 0, den)
    assert not (tmp_path / "missing.h5").exists()
    # ... then the valid call, and a second one finds the datasets there and leaves the file as the first made it
    host.write_values(path, db, queries, protein_lut, k, value, 1, 0, 0, den, vrect)
    image = path.read_bytes()
    with pytest.raises(HostError, match="already holds /hit_values"):
        host.write_values(path, db, queries, protein_lut, k, value, 1, 0, 0, den, vrect)
    assert path.read_bytes() == image
