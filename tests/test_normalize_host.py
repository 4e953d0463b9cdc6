"""CPU: the host-only side of the normalised scores through the binding (sa_norm_value against Python's integers; the argument
checks of the device calls that come before any device is looked for: null pointers, a source or a rule outside its enum, each
through sa_last_error with nothing written and followed by a call that works), sa_host_write_normalization of cli/libsa_host.so
(the writer of --normalize) through ctypes: /normalization_denominators (N I32LE), /normalization_rule (2 I32LE) and
/normalization_scale (1 I32LE), added to a finished file without touching what is in it; and the tool's option errors, which need
no device."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF, ROOT, Host, HostError, _Store, h5_matrix, h5_sequences
from tests.linkage_ref import random_full
from tests.test_edges_host import h5_array, h5_header
from tests.test_neighbors_host import h5_names

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
SCALE = 1000000
NORM_SETS = ("/normalization_denominators", "/normalization_rule", "/normalization_scale")
POISON = -0x5A5A5A5B


def python_value(s: int, di: int, dj: int, rule: int) -> int:
    """the contract of include/seqalign_hip.h, with Python's integers"""
    den, num = (min(di, dj), s * SCALE) if rule == 0 else (max(di, dj), s * SCALE) if rule == 1 else (di + dj, 2 * s * SCALE)
    if den <= 0:
        return INT32_MIN
    return max(INT32_MIN, min(INT32_MAX, num // den))


# ---- the library's host-only calls ---------------------------------------------------------------------------------------------
def test_constants(sa):
    assert (sa.NORM_SELF, sa.NORM_LENGTH) == (0, 1) and (sa.NORM_MIN, sa.NORM_MAX, sa.NORM_MEAN) == (0, 1, 2) and sa.NORM_SCALE == SCALE
    assert sa.load_library().sa_abi_version() == 4  # additions only


def test_norm_value_is_pythons_floor_division(sa):
    grid = [INT32_MIN, INT32_MIN + 1, -SCALE, -1, 0, 1, 2, 3, SCALE - 1, SCALE, SCALE + 1, INT32_MAX - 1, INT32_MAX]
    for rule in (0, 1, 2):
        for s in grid:
            for di in grid:
                for dj in grid:
                    assert sa.norm_value(s, di, dj, rule) == python_value(s, di, dj, rule), (s, di, dj, rule)
    rng = np.random.default_rng(5)
    triples = np.concatenate([rng.integers(INT32_MIN, INT32_MAX, (3000, 3), endpoint=True),
                              np.stack([rng.integers(-100000, 100000, 3000), rng.integers(-5, 3000, 3000), rng.integers(-5, 3000, 3000)], 1)])
    inexact = 0
    for s, di, dj in triples.tolist():
        for rule in (0, 1, 2):
            assert sa.norm_value(s, di, dj, rule) == python_value(s, di, dj, rule), (s, di, dj, rule)
        inexact += s < 0 and min(di, dj) > 0 and (s * SCALE) % min(di, dj) != 0
    assert inexact > 500  # negative quotients that are no exact multiples: the floor rule, not truncation
    assert sa.norm_value(-1, 3, 3, sa.NORM_MIN) == -333334 and sa.norm_value(1, 3, 3, sa.NORM_MIN) == 333333


@pytest.mark.parametrize("rule", [-1, 3, 17, INT32_MIN, INT32_MAX])
def test_norm_value_refuses_a_rule_outside_the_enum(rule, sa):
    lib = sa.load_library()
    with pytest.raises(sa.AlignError, match=f"rule {rule} is none of"):
        sa.norm_value(5, 7, 7, rule)
    assert lib.sa_norm_value(5, 7, 7, rule) == INT32_MIN and b"sa_norm_value" in lib.sa_last_error()
    assert sa.norm_value(5, 7, 7, sa.NORM_MAX) == 714285  # ... and the library goes on working
    with pytest.raises(sa.AlignError, match="int32"):
        sa.norm_value(2**31, 1, 1, 0)


def small_case(sa):
    from tests.synth import make_protein_set
    return sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3)), sa.Scoring.from_names("nw", "blosum62", gap_pen=4)


ONE_CALLS = ["neighbors", "edges", "linkage", "select", "edges_at_rank", "linkage_with_ranks"]


def one_call(sa, which, store, scoring, norm):
    return {"neighbors": lambda: sa.hip_neighbors(store, scoring, 2, norm=norm),
            "edges": lambda: sa.hip_edges(store, scoring, 0, norm=norm),
            "linkage": lambda: sa.hip_linkage(store, scoring, norm=norm),
            "select": lambda: sa.hip_select(store, scoring, [0, 9], norm=norm),
            "edges_at_rank": lambda: sa.hip_edges_at_rank(store, scoring, 5, norm=norm),
            "linkage_with_ranks": lambda: sa.hip_linkage_with_ranks(store, scoring, [0, 9], norm=norm)}[which]()


@pytest.mark.parametrize("which", ONE_CALLS)
@pytest.mark.parametrize("source,rule,message", [(2, 0, "source 2 is neither"), (-1, 1, "source -1 is neither"), (0, 3, "rule 3 is none of"),
                                                 (1, -1, "rule -1 is none of")])
def test_one_call_variants_refuse_a_bad_norm_before_a_device_is_looked_for(which, source, rule, message, sa):
    store, scoring = small_case(sa)
    with pytest.raises(sa.AlignError, match=f"sa_hip_{which}_norm: {message}"):
        one_call(sa, which, store, scoring, sa.Norm(source, rule))
    assert sa.norm_value(6, 3, 2, sa.NORM_MEAN) == 2400000  # ... and the library goes on working


def test_null_arguments_are_refused_with_nothing_written(sa):
    from sequencealigner_amd.binding import _Norm
    lib = sa.load_library()
    store, scoring = small_case(sa)
    sc, inp = scoring._as_c(), store._as_c()
    den = np.full(5, POISON, np.int32)
    out = np.full(64, POISON, np.int32)
    out64 = np.full(8, POISON, np.int64)
    ranks = np.zeros(1, np.int64)
    good = _Norm(0, 0, den.ctypes.data)
    o, o64, r = out.ctypes.data, out64.ctypes.data, ranks.ctypes.data

    def refused(result, what="null"):
        assert not result and what.encode() in lib.sa_last_error(), lib.sa_last_error()
        assert sa.norm_value(1, 1, 1, 0) == SCALE  # a valid call after every refusal

    refused(lib.sa_ctx_denominators(None, 0, o, None) == 0)
    refused(lib.sa_ctx_normalize(None, o, o, 0, o, None) == 0)
    refused(lib.sa_zjob_normalize(None, C.byref(good)) == 0)
    refused(lib.sa_hip_neighbors_norm(inp, None, 2, o, o, C.byref(good)))
    refused(lib.sa_hip_neighbors_norm(inp, C.byref(sc), 2, None, o, C.byref(good)))
    refused(lib.sa_hip_neighbors_norm(inp, C.byref(sc), 2, o, None, C.byref(good)))
    refused(lib.sa_hip_edges_norm(inp, None, 0, C.byref(good)))
    refused(lib.sa_hip_linkage_norm(inp, None, C.byref(good)))
    refused(lib.sa_hip_select_norm(inp, None, r, 1, o, o64, C.byref(good)))
    refused(lib.sa_hip_select_norm(inp, C.byref(sc), None, 1, o, o64, C.byref(good)))
    refused(lib.sa_hip_select_norm(inp, C.byref(sc), r, 1, None, o64, C.byref(good)))
    refused(lib.sa_hip_select_norm(inp, C.byref(sc), r, 1, o, None, C.byref(good)))
    cut, below = C.c_int32(POISON), C.c_int64(POISON)
    refused(lib.sa_hip_edges_at_rank_norm(inp, None, 0, C.byref(cut), C.byref(below), C.byref(good)))
    refused(lib.sa_hip_edges_at_rank_norm(inp, C.byref(sc), 0, None, C.byref(below), C.byref(good)))
    refused(lib.sa_hip_linkage_with_ranks_norm(inp, None, r, 1, o, o64, C.byref(good)))
    refused(lib.sa_hip_linkage_with_ranks_norm(inp, C.byref(sc), r, 1, None, o64, C.byref(good)))
    # the messages name the entry point that was called
    assert not lib.sa_hip_edges_norm(inp, None, 0, C.byref(good)) and b"sa_hip_edges_norm" in lib.sa_last_error()
    assert not lib.sa_hip_edges(inp, None, 0) and b"sa_hip_edges:" in lib.sa_last_error()
    assert (den == POISON).all() and (out == POISON).all() and (out64 == POISON).all() and cut.value == POISON and below.value == POISON


def test_norm_wants_int32_values(sa):
    with pytest.raises(sa.AlignError, match="int32"):
        sa.Norm(2**31, 0)
    with pytest.raises(sa.AlignError, match="int32"):
        sa.Norm(0, -2**31 - 1)
    n = sa.Norm()
    assert (n.source, n.rule) == (sa.NORM_SELF, sa.NORM_MIN) and "source=0" in repr(n)


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class NormalizeHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_normalization.argtypes = [C.c_char_p, C.POINTER(_Store), C.c_void_p, C.c_int32, C.c_int32]
        self.lib.sa_host_write_normalization.restype = C.c_int

    def write_normalization(self, path, seqs, lut, den, source, rule):
        st = self.parse(b"".join(b">s\n" + s + b"\n" for s in seqs), "fasta", lut)
        try:
            den = None if den is None else np.ascontiguousarray(den, np.int32)
            if self.lib.sa_host_write_normalization(str(path).encode(), C.byref(st), None if den is None else den.ctypes.data, int(source), int(rule)):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(st))


@pytest.fixture(scope="module")
def host():
    return NormalizeHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, seed):
    from tests.synth import make_protein_set
    seqs = make_protein_set(n, 8, 20, seed)
    den = np.random.default_rng(seed).integers(-3, 5000, n).astype(np.int32)
    return seqs, random_full(n, 400, seed), den


def assert_written(path, den, source, rule):
    assert np.array_equal(h5_array(path, "normalization_denominators", "<i4"), den)
    assert h5_array(path, "normalization_rule", "<i4").tolist() == [source, rule]
    assert h5_array(path, "normalization_scale", "<i4").tolist() == [SCALE]
    for name, extent in (("/normalization_denominators", f"( {len(den)} )"), ("/normalization_rule", "( 2 )"), ("/normalization_scale", "( 1 )")):
        props = h5_header(path, name)
        assert "H5T_STD_I32LE" in props and extent in props and "CONTIGUOUS" in props, props


@pytest.mark.parametrize("n,compression,source,rule", [(40, 0, 0, 0), (300, 0, 1, 2), (300, 4, 0, 1)])
def test_datasets_are_added_to_a_finished_file(n, compression, source, rule, host, protein_lut, tmp_path):
    seqs, matrix, den = case(n, 5)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, compression)
    shutil.copy(path, before)
    host.write_normalization(path, seqs, protein_lut, den, source, rule)
    assert h5_names(path) == {"/sequences", "/similarity_matrix", *NORM_SETS}
    assert_written(path, den, source, rule)
    for name in ("/similarity_matrix", "/sequences"):
        res = subprocess.run([str(H5DIFF), str(before), str(path), name], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(h5_matrix(path, n), matrix) and h5_sequences(path) == seqs


def test_bad_arguments_are_an_error_and_touch_nothing(host, protein_lut, tmp_path):
    n = 30
    seqs, matrix, den = case(n, 8)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, 0)
    shutil.copy(path, before)
    for d, source, rule, message in ((None, 0, 0, "missing"), (den, 2, 0, "source 2"), (den, -1, 0, "source -1"), (den, 0, 3, "rule 3"),
                                     (den, 1, -1, "rule -1")):
        with pytest.raises(HostError, match=message):
            host.write_normalization(path, seqs, protein_lut, d, source, rule)
        assert path.read_bytes() == before.read_bytes()
    host.write_normalization(path, seqs, protein_lut, den, 1, 1)  # ... and the library goes on working
    assert_written(path, den, 1, 1)


def test_appending_to_a_missing_file_is_an_error(host, protein_lut, tmp_path):
    seqs, _, den = case(20, 9)
    with pytest.raises(HostError, match="Failed to open"):
        host.write_normalization(tmp_path / "nothing.h5", seqs, protein_lut, den, 0, 0)
    assert not (tmp_path / "nothing.h5").exists()


# ---- the tool's option errors ---------------------------------------------------------------------------------------------------
REFUSED = [
    (["--normalize", "self-min"], "--normalize requires something selected from the scores"),
    (["--normalize", "len-mean", "--alignments"], "--alignments requires -k"),
    (["--normalize", "self"], "Normalization rule must be one of self-min"),
    (["--normalize", "SELF-MIN", "-k", "2"], "Normalization rule must be one of self-min"),
    (["--normalize", "", "-k", "2"], "Normalization rule must be one of self-min"),
    (["--normalize", "geo-mean", "--linkage"], "Normalization rule must be one of self-min"),
    (["-k", "2", "--normalize"], "--normalize requires a parameter"),
]


@pytest.mark.parametrize("bad,message", REFUSED)
def test_option_errors_leave_no_output(bad, message, tmp_path):
    """refused while the options are read: before any input is loaded and before a device is looked for"""
    cli = ROOT / "cli" / "seqalign"
    if not cli.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    fasta, out = tmp_path / "in.fasta", tmp_path / "out.h5"
    fasta.write_bytes(b">a\nARNDCQEG\n>b\nARNDCQEGHIL\n>c\nHILKMFPSTW\n")
    res = subprocess.run([str(cli), "-i", str(fasta), "-o", str(out), "-a", "nw", "-m", "blosum62", "-p", "4", "-F", *bad],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and message in res.stderr and "usage information" in res.stderr, res.stdout + res.stderr
    assert not out.exists()


def test_help_documents_the_option():
    cli = ROOT / "cli" / "seqalign"
    if not cli.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--normalize RULE", "self-min", "len-mean", "STAYS RAW", "/normalization_denominators", "/normalization_rule",
                 "/normalization_scale", "parts per million"):
        assert word in text, word
