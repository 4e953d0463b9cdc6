"""CPU: what the threshold search (csrc/sa_search_above.hip, --hits-min) needs no device for.
  - Every refusal of sa_hip_search_above and of the two context calls that comes before a device is looked for, with its message,
    each followed by a valid host-only call; with everything valid the call gets as far as the device.  (The refusals that need a
    context are in tests/test_gpu_search_above.py.)
  - The scratch size on the host: 8 * (nq * S + 1) with the S of the segment rule.
  - The tool: --hits-min without --query, with -k, a T that is no integer, --help; the refusals tests/test_search_cli_host.py pins still
    hold beside the new option.
  - sa_host_write_search_list of cli/libsa_host.so through ctypes: every dataset exact through h5dump, E = 0, each bad input an error
    and no file."""
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


# ---- the library ---------------------------------------------------------------------------------------------------------------
def still_answers(sa):
    """a valid call after a refusal: host-only, exact"""
    assert sa.norm_value(-7, 3, 5, sa.NORM_MIN) == (-7 * 1000000) // 3
    assert sa.hits_above_scratch_bytes(130, 4) == 8 * (4 * 2 + 1)


def test_scratch_size_follows_the_segment_rule(sa):
    # S = 1 when the rows fill the device (2048); otherwise min(ceil(8192 / nq), max(1, N / 64))
    for n, nq, s in ((1, 5, 1), (65, 3, 1), (127, 3, 1), (128, 4, 2), (130, 4, 2), (200_003, 2, 3125), (70, 3000, 1), (10**6, 3, 2731),
                     (10**6, 2047, 5), (10**6, 2048, 1), (2**31 - 1, 1, 8192), (2**31 - 1, 2**31 - 1, 1)):
        assert sa.hits_above_scratch_bytes(n, nq) == 8 * (nq * s + 1), (n, nq)
    for n, nq in ((0, 1), (1, 0), (-1, 5), (5, -1), (-2**31, -2**31)):
        assert sa.hits_above_scratch_bytes(n, nq) == 0


def test_context_calls_refuse_a_null_context(sa):
    lib = sa.load_library()
    for call, name in ((lambda: lib.sa_ctx_hits_above_offsets(None, None, 1, 0, None, None, None), "sa_ctx_hits_above_offsets"),
                       (lambda: lib.sa_ctx_hits_above_fill(None, None, None, 1, 0, None, None, None, None, None, None), "sa_ctx_hits_above_fill")):
        assert call() != 0
        assert lib.sa_last_error().decode() == f"{name}: null context"
        still_answers(sa)


def test_the_one_call_form_refuses_before_a_device_is_looked_for(sa):
    lib = sa.load_library()
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    db = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    queries = sa.SequenceStore.from_sequences(make_protein_set(3, 8, 12, 4))
    empty = sa.SequenceStore.from_sequences([])
    sc = scoring._as_c()
    den = np.full(8, 77, np.int32)
    cn = sa.binding._Norm(sa.NORM_SELF, sa.NORM_MIN, den.ctypes.data)

    def call(a=db, b=queries, s=C.byref(sc), t=0, norm=None, denom=None):
        cd = None if denom is None else C.c_int32(denom)
        return lib.sa_hip_search_above(a._as_c() if hasattr(a, "_as_c") else a, b._as_c() if hasattr(b, "_as_c") else b, s, t,
                                       None if norm is None else C.byref(norm), None if cd is None else C.byref(cd))

    def reaches_the_device(**kw):
        if sa.device_count() == 0:
            assert not call(**kw) and b"No HIP devices" in lib.sa_last_error()

    def refused(message, **kw):
        assert not call(**kw)
        text = lib.sa_last_error().decode()
        assert text.startswith("sa_hip_search_above: ") and message in text, text
        still_answers(sa)
        reaches_the_device()

    refused("null argument", s=None)
    refused("norm and pid_denom exclude each other", norm=cn, denom=sa.PID_COLUMNS)
    refused("empty store", a=empty)
    refused("empty store", b=empty)
    refused("null sequence store", a=sa.binding._Input(None, None, 0, 5))
    refused("null sequence store", b=sa.binding._Input(None, None, 0, 3))
    for source, rule, message in ((2, 0, "source 2 is neither"), (-1, 0, "source -1 is neither"), (0, 3, "rule 3 is none of"), (0, -1, "rule -1 is none of")):
        refused(message, norm=sa.binding._Norm(source, rule, den.ctypes.data))
    for denom in (-1, 4, 2 ** 31 - 1):
        refused(f"denom {denom} is none of", denom=denom)
    assert (den == 77).all(), "a refused call wrote to its outputs"
    # any int32 threshold and every quantity are valid arguments
    for kw in (dict(t=-2**31), dict(t=2**31 - 1), dict(norm=cn), dict(denom=sa.PID_SHORTER)):
        reaches_the_device(**kw)
    # the accessors of a NULL list
    m, count = C.c_int32(7), C.c_int64(7)
    assert lib.sa_hitlist_offsets(None, C.byref(m)) is None and lib.sa_hitlist_index(None, C.byref(count)) is None
    assert (m.value, count.value) == (0, 0) and lib.sa_hitlist_value(None) is None and lib.sa_hitlist_score(None) is None
    lib.sa_hitlist_destroy(None)
    assert sa.last_search_above_seconds() >= 0.0


def test_binding_refusals(sa):
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    db = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))
    queries = sa.SequenceStore.from_sequences(make_protein_set(3, 8, 12, 4))
    with pytest.raises(sa.AlignError, match="sa_hip_search_above: norm and pid_denom exclude each other"):
        sa.hip_search_above(db, queries, scoring, 0, norm=sa.Norm(), pid=sa.PID_COLUMNS)
    with pytest.raises(sa.AlignError, match="min_value = 2147483648 is not an int32"):
        sa.hip_search_above(db, queries, scoring, 2**31)
    with pytest.raises(sa.AlignError, match="sa_hip_search_above: rule 5"):
        sa.hip_search_above(db, queries, scoring, 0, norm=sa.Norm(sa.NORM_LENGTH, 5))
    still_answers(sa)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return exe


REFUSED = [
    (["--hits-min", "5"], "--hits-min requires --query"),
    (["--hits-min", "5", "--hits-by", "self-min"], "--hits-by requires --query"),
    (["--query", "Q", "--hits-min", "5", "-k", "2"], "--hits-min and -k, --neighbors conflict"),
    (["--query", "Q", "-k", "2", "--hits-by", "identity-shorter", "--hits-min", "900000"], "--hits-min and -k, --neighbors conflict"),
    (["--query", "Q", "--hits-min", "5.5"], "Hit threshold must be an integer between -2147483648 and 2147483647"),
    (["--query", "Q", "--hits-min", "five"], "Hit threshold must be an integer between -2147483648 and 2147483647"),
    (["--query", "Q", "--hits-min", "2147483648"], "Hit threshold must be an integer between -2147483648 and 2147483647"),
    (["--query", "Q", "--hits-min", ""], "Hit threshold must be an integer between -2147483648 and 2147483647"),
    # what tests/test_search_cli_host.py pins, beside the new option as well
    (["--query", "Q"], "--query requires -k"),
    (["--query", "Q", "--hits-min", "5", "--min-score", "5"], "--query and --min-score conflict"),
    (["--query", "Q", "--hits-min", "5", "--neighbors-only"], "--query and --neighbors-only conflict"),
    (["--query", "Q", "--hits-min", "5", "--normalize", "self-min"], "--query and --normalize conflict"),
    (["--query", "Q", "--hits-min", "5", "-z", "3"], "--query and -z, --compression conflict"),
    (["--alignments", "--hits-min", "5"], "--hits-min requires --query"),
    (["--alignments"], "--alignments requires -k"),
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


@pytest.mark.parametrize("extra", [[], ["--alignments"], ["--query-scores"], ["--hits-by", "identity-shorter"], ["--hits-by", "score"]])
def test_accepted_options_get_as_far_as_the_device(extra, cli, tmp_path, sa):
    """--hits-min stands in for -k, any int32, with --alignments as well: without a device the run ends at the library's message"""
    if sa.device_count() != 0:
        return  # (a device is present: tests/test_gpu_search_above_cli.py runs these to the end)
    fasta, queries, out = tmp_path / "in.fasta", tmp_path / "q.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nARNDCQEG\n>b\nARNDCQEGHIL\n>c\nHILKMFPSTW\n")
    queries.write_bytes(b">x\nARNDCQ\n>y\nHILKMF\n")
    for t in ("-2147483648", "0", "2147483647"):
        res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-a", "nw", "-m", "blosum62", "-p", "4", "-F", "-P",
                              "--query", str(queries), "--hits-min", t, *extra], capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and "No HIP devices" in res.stderr and "usage information" not in res.stderr, res.stdout + res.stderr
        assert not out.exists()


def test_help_documents_the_option(cli):
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--hits-min T", "in place of -k", "/hitlist_offsets", "/hitlist_indices", "/hitlist_scores", "/hitlist_min", "/hitlist_values",
                 "/hitlist_alignment_records", "/hitlist_cigar_offsets", "/hitlist_cigars", "ASCENDING", "second alignment",
                 "--hits-by identity-shorter --hits-min 900000", "parts per million"):
        assert word in text, word


# ---- the writer ----------------------------------------------------------------------------------------------------------------
class ListHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_search_list.argtypes = [C.c_char_p, C.POINTER(_Store), C.POINTER(_Store), C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        self.lib.sa_host_write_search_list.restype = C.c_int

    def write_list(self, path, db, queries, lut, offsets, index, score, t, value=None, kind=0, source=0, rule=0, den=None, rect=None, vrect=None,
                   records=None, cigar=None):
        sd = self.parse(b"".join(b">s\n" + s + b"\n" for s in db), "fasta", lut)
        sq = self.parse(b"".join(b">s\n" + s + b"\n" for s in queries), "fasta", lut)
        try:
            keep = [np.ascontiguousarray(offsets, np.int64)] + [None if a is None else np.ascontiguousarray(a, np.int32)
                                                                for a in (index, score, value, den, rect, vrect)]
            cigar = None if cigar is None else np.ascontiguousarray(cigar, np.uint32)
            ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
            o, i, s, v, d, r, vr = keep
            if self.lib.sa_host_write_search_list(str(path).encode(), C.byref(sd), C.byref(sq), o.ctypes.data, ptr(i), ptr(s), int(t), ptr(v),
                                                  kind, source, rule, ptr(d), ptr(r), ptr(vr), int(records is not None), ptr(records),
                                                  ptr(cigar), 0 if cigar is None else cigar.size):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(sd))
            self.lib.sa_host_store_free(C.byref(sq))


@pytest.fixture(scope="module")
def host():
    return ListHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, m, seed, empty=False):
    """a CSR with an empty row, a full row and rows between; everything else random"""
    rng = np.random.default_rng(seed)
    db, queries = make_protein_set(n, 8, 30, seed), make_protein_set(m, 8, 30, seed + 1)
    counts = rng.integers(0, n + 1, m)
    counts[0], counts[-1] = 0, n
    if empty:
        counts[:] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    e = int(offsets[-1])
    index = np.concatenate([np.sort(rng.permutation(n)[:c]) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    score, value = (rng.integers(-2**31, 2**31 - 1, e, dtype=np.int64).astype(np.int32) for _ in range(2))
    den = rng.integers(-5, 4000, n + m).astype(np.int32)
    rect, vrect = (rng.integers(-2**31, 2**31 - 1, (m, n), dtype=np.int64).astype(np.int32) for _ in range(2))
    records = np.zeros(e, ALN)
    for f in ALN.names[:7]:
        records[f] = rng.integers(0, 1000, e)
    records["cigar_len"] = rng.integers(0, 4, e)
    records["cigar_off"] = np.concatenate([[0], np.cumsum(records["cigar_len"])[:-1]]) if e else records["cigar_off"]
    cigar = rng.integers(0, 2**32 - 1, int(records["cigar_len"].sum()), dtype=np.int64).astype(np.uint32)
    return dict(db=db, queries=queries, offsets=offsets, index=index, score=score, value=value, den=den, rect=rect, vrect=vrect, records=records,
                cigar=cigar)


BASE = {"/sequences", "/query_sequences", "/hitlist_offsets", "/hitlist_indices", "/hitlist_scores", "/hitlist_min"}


def check_base(path, c, t):
    assert h5_strings(path, "sequences") == c["db"] and h5_strings(path, "query_sequences") == c["queries"]
    assert np.array_equal(h5_array(path, "hitlist_offsets", "<i8"), c["offsets"])
    assert np.array_equal(h5_array(path, "hitlist_indices", "<i4"), c["index"])
    assert np.array_equal(h5_array(path, "hitlist_scores", "<i4"), c["score"])
    assert h5_array(path, "hitlist_min", "<i4").tolist() == [t]


@pytest.mark.parametrize("n,m,t", [(40, 7, 17), (2, 2, -2**31), (300, 20, 2**31 - 1)])
def test_raw_scores_alone(n, m, t, host, protein_lut, tmp_path):
    c = case(n, m, 5)
    path = tmp_path / "l.h5"
    host.write_list(path, c["db"], c["queries"], protein_lut, c["offsets"], c["index"], c["score"], t, value=c["value"], vrect=c["vrect"])
    assert h5_names(path) == BASE  # (kind 0: the value arrays are not looked at)
    check_base(path, c, t)


@pytest.mark.parametrize("kind,source,rule", [(1, 0, 0), (1, 1, 2), (2, 0, 1), (2, 0, 3)])
def test_everything_under_a_quantity(kind, source, rule, host, protein_lut, tmp_path):
    n, m, t = 40, 7, 900000
    c = case(n, m, 6)
    path = tmp_path / "l.h5"
    host.write_list(path, c["db"], c["queries"], protein_lut, c["offsets"], c["index"], c["score"], t, c["value"], kind, source, rule, c["den"],
                    c["rect"], c["vrect"], c["records"], c["cigar"])
    want = BASE | {"/hitlist_values", "/hit_quantity", "/hit_scale", "/hitlist_alignment_records", "/hitlist_cigar_offsets", "/hitlist_cigars",
                   "/query_scores", "/query_values"} | ({"/database_denominators", "/query_denominators"} if kind == 1 else set())
    assert h5_names(path) == want
    check_base(path, c, t)
    e = len(c["index"])
    assert np.array_equal(h5_array(path, "hitlist_values", "<i4"), c["value"])
    assert h5_array(path, "hit_quantity", "<i4").tolist() == [kind, source if kind == 1 else 0, rule]
    assert h5_array(path, "hit_scale", "<i4").tolist() == [1000000]
    if kind == 1:
        assert np.array_equal(h5_array(path, "database_denominators", "<i4"), c["den"][:n])
        assert np.array_equal(h5_array(path, "query_denominators", "<i4"), c["den"][n:])
    assert np.array_equal(h5_array(path, "query_scores", "<i4").reshape(m, n), c["rect"])
    assert np.array_equal(h5_array(path, "query_values", "<i4").reshape(m, n), c["vrect"])
    fields = h5_array(path, "hitlist_alignment_records", "<i4").reshape(e, 8)
    for k, f in enumerate(ALN.names[:8]):
        assert np.array_equal(fields[:, k], c["records"][f]), f
    assert np.array_equal(h5_array(path, "hitlist_cigar_offsets", "<i8"), np.concatenate([c["records"]["cigar_off"], [c["cigar"].size]]))
    assert np.array_equal(h5_array(path, "hitlist_cigars", "<u4"), c["cigar"])


def test_alignments_without_a_quantity_and_rectangle_without_alignments(host, protein_lut, tmp_path):
    c = case(30, 5, 7)
    path = tmp_path / "l.h5"
    host.write_list(path, c["db"], c["queries"], protein_lut, c["offsets"], c["index"], c["score"], 3, records=c["records"], cigar=c["cigar"])
    assert h5_names(path) == BASE | {"/hitlist_alignment_records", "/hitlist_cigar_offsets", "/hitlist_cigars"}
    host.write_list(path, c["db"], c["queries"], protein_lut, c["offsets"], c["index"], c["score"], 3, rect=c["rect"], vrect=c["vrect"])
    assert h5_names(path) == BASE | {"/query_scores"}  # (a new file each time; no /query_values without a quantity)
    check_base(path, c, 3)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_no_hit_at_all(kind, host, protein_lut, tmp_path):
    """E = 0: the datasets are there with extent 0, the offsets all 0; the arrays may be NULL"""
    n, m = 12, 4
    c = case(n, m, 8, empty=True)
    assert c["offsets"].tolist() == [0] * (m + 1) and c["index"].size == 0
    path = tmp_path / "l.h5"
    host.write_list(path, c["db"], c["queries"], protein_lut, c["offsets"], None, None, 2**31 - 1, None, kind, 0, 0, c["den"] if kind == 1 else None,
                    records=c["records"], cigar=None)
    names = h5_names(path)
    assert BASE | {"/hitlist_alignment_records", "/hitlist_cigar_offsets", "/hitlist_cigars"} <= names
    assert ("/hitlist_values" in names) == (kind != 0) and ("/database_denominators" in names) == (kind == 1)
    for name, dt in (("hitlist_indices", "<i4"), ("hitlist_scores", "<i4"), ("hitlist_alignment_records", "<i4"), ("hitlist_cigars", "<u4")):
        assert h5_array(path, name, dt).size == 0, name
    if kind:
        assert h5_array(path, "hitlist_values", "<i4").size == 0
    assert h5_array(path, "hitlist_offsets", "<i8").tolist() == [0] * (m + 1)
    assert h5_array(path, "hitlist_cigar_offsets", "<i8").tolist() == [0]
    assert h5_array(path, "hitlist_min", "<i4").tolist() == [2**31 - 1]


def test_bad_inputs_are_errors_and_no_file(host, protein_lut, tmp_path):
    n, m = 10, 4
    c = case(n, m, 9)
    path = tmp_path / "l.h5"

    def write(**kw):
        a = dict(offsets=c["offsets"], index=c["index"], score=c["score"], t=0, value=c["value"], kind=0, source=0, rule=0, den=c["den"])
        a.update(kw)
        host.write_list(path, c["db"], c["queries"], protein_lut, a["offsets"], a["index"], a["score"], a["t"], a["value"], a["kind"], a["source"],
                        a["rule"], a["den"])

    off = c["offsets"].copy()
    off[0] = 1
    down = c["offsets"].copy()
    down[1], down[2] = 3, 2
    outside_lo, outside_hi, unsorted, twice = (c["index"].copy() for _ in range(4))
    last = int(c["offsets"][m]) - 1  # (the last row is full: 0 .. n - 1)
    outside_lo[last - 3], outside_hi[last], unsorted[[last - 1, last]], twice[last] = -1, n, unsorted[[last, last - 1]], twice[last - 1]
    bad = [("Hit list offsets must start at 0", dict(offsets=off)),
           ("Hit list offsets decrease at query 1", dict(offsets=down)),
           (f"Hit index -1 of query {m - 1} outside the 10 database sequences", dict(index=outside_lo)),
           (f"Hit index 10 of query {m - 1} outside the 10 database sequences", dict(index=outside_hi)),
           (f"Hit indices of query {m - 1} are not in ascending order", dict(index=unsorted)),
           (f"Hit indices of query {m - 1} are not in ascending order", dict(index=twice)),
           ("Hit list data missing", dict(index=None)),
           ("Hit list data missing", dict(score=None)),
           ("Hit list data missing", dict(kind=2, value=None)),
           ("Hit list data missing", dict(kind=1, den=None)),
           ("Hit quantity kind 3 is none of", dict(kind=3)),
           ("Hit quantity kind -1 is none of", dict(kind=-1)),
           ("Normalization source 2 is neither", dict(kind=1, source=2)),
           ("Normalization rule 3 is none of", dict(kind=1, rule=3)),
           ("Identity denominator 4 is none of", dict(kind=2, rule=4))]
    for message, kw in bad:
        with pytest.raises(HostError, match=message):
            write(**kw)
        assert not path.exists(), message
    write()
    check_base(path, c, 0)
