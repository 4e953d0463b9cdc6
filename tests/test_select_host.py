"""CPU: the host-only calls of the score order statistics through the binding (sa_score_rank, sa_select_scratch_bytes, and the
argument checks of the device calls that come before any device is looked for), sa_host_write_quantiles of cli/libsa_host.so
(the writer of --min-quantile / --clusters-quantile / --quantiles) through ctypes: /score_quantiles (m F64LE),
/score_quantile_values (m I32LE), /score_quantile_below (m I64LE), /edge_min_score and /cluster_min_score (1 I32LE), added to a
finished file without touching what is in it, or written with /sequences alone; and the tool's option errors, which need no
device."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF, ROOT, Host, HostError, _Store, h5_matrix, h5_sequences
from tests.linkage_ref import random_full
from tests.test_edges_host import h5_array, h5_header
from tests.test_neighbors_host import h5_names

QUANTILE_SETS = ("/score_quantiles", "/score_quantile_values", "/score_quantile_below")


# ---- the library's host-only calls ---------------------------------------------------------------------------------------------
def python_rank(pairs, q):
    if pairs < 1 or math.isnan(q) or not 0.0 <= q <= 1.0:
        return -1
    return min(pairs - 1, int(q * pairs))


@pytest.mark.parametrize("pairs", [1, 2, 3, 100, 4950, 49_995_000, 4_999_950_000, 2 ** 40 + 1])
def test_score_rank_is_the_python_rule(pairs, sa):
    for q in (0.0, 1.0, 0.5, 0.99, 0.98, 0.999, 1 / 3, 0.1, 1e-12, 1 - 1e-12, float("nan"), -0.1, 1.5, float("inf"), -0.0):
        assert sa.score_rank(pairs, q) == python_rank(pairs, q), (pairs, q)
    assert sa.score_rank(pairs, 0.0) == 0 and sa.score_rank(pairs, 1.0) == pairs - 1  # the minimum and the maximum


def test_score_rank_refuses_what_is_no_fraction_or_no_matrix(sa):
    assert [sa.score_rank(100, q) for q in (float("nan"), -0.1, 1.5)] == [-1, -1, -1]
    assert sa.score_rank(0, 0.5) == -1 and sa.score_rank(-7, 0.5) == -1
    assert sa.score_rank(100, 0.99) == int(0.99 * 100) == 99 and sa.score_rank(100, 0.98) == 98  # (the IEEE product: 0.99 * 100 == 99.0)


def test_scratch_bytes(sa):
    assert sa.select_scratch_bytes(0) == 0 and sa.select_scratch_bytes(17) == 0 and sa.select_scratch_bytes(-1) == 0
    sizes = [sa.select_scratch_bytes(m) for m in range(1, 17)]
    assert all(b % 8 == 0 for b in sizes) and all(b - a == 256 * 8 for a, b in zip(sizes, sizes[1:]))  # one 64-bit table per rank
    assert 256 * 8 < sizes[0] < 256 * 8 + 1024


def test_bad_calls_are_refused_before_a_device_is_looked_for(sa):
    """m, N, the ranks and null pointers: through sa_last_error, nothing written"""
    from tests.synth import make_protein_set
    lib = sa.load_library()
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    store = sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3))  # P = 10
    one = sa.SequenceStore.from_sequences(make_protein_set(1, 8, 12, 3))
    for ranks, message in (([-1], "outside"), ([10], "outside"), ([0, 3, 10], "outside"), ([], "ranks|null"), (list(range(10)) + [0] * 7, "17 ranks")):
        with pytest.raises(sa.AlignError, match=message):
            sa.hip_select(store, scoring, ranks)
        with pytest.raises(sa.AlignError, match=message):
            sa.hip_linkage_with_ranks(store, scoring, ranks)
    for rank in (-1, 10):
        with pytest.raises(sa.AlignError, match="outside"):
            sa.hip_edges_at_rank(store, scoring, rank)
    with pytest.raises(sa.AlignError, match="no pair"):
        sa.hip_select(one, scoring, [0])
    sc = scoring._as_c()
    ranks, value, below = np.zeros(1, np.int64), np.full(1, 77, np.int32), np.full(1, 77, np.int64)
    for args in ((None, 1, value.ctypes.data, below.ctypes.data), (ranks.ctypes.data, 1, None, below.ctypes.data),
                 (ranks.ctypes.data, 1, value.ctypes.data, None)):
        assert not lib.sa_hip_select(store._as_c(), C.byref(sc), *args) and b"null" in lib.sa_last_error()
    assert lib.sa_zjob_select(None, ranks.ctypes.data, 1, value.ctypes.data, below.ctypes.data) != 0 and b"null" in lib.sa_last_error()
    assert lib.sa_ctx_select(None, None, ranks.ctypes.data, 1, None, None, None, None) != 0 and b"null" in lib.sa_last_error()
    assert value[0] == 77 and below[0] == 77


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class SelectHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_quantiles.argtypes = [C.c_char_p, C.POINTER(_Store), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                     C.c_void_p, C.c_void_p, C.c_int]
        self.lib.sa_host_write_quantiles.restype = C.c_int

    def write_quantiles(self, path, seqs, lut, fractions, values, below, edge_min, cluster_min, create):
        st = self.parse(b"".join(b">s\n" + s + b"\n" for s in seqs), "fasta", lut)
        try:
            fractions = np.ascontiguousarray(fractions, np.float64)
            values = np.ascontiguousarray(values, np.int32)
            below = np.ascontiguousarray(below, np.int64)
            e = None if edge_min is None else np.array([edge_min], np.int32)
            c = None if cluster_min is None else np.array([cluster_min], np.int32)
            if self.lib.sa_host_write_quantiles(str(path).encode(), C.byref(st), fractions.ctypes.data, values.ctypes.data, below.ctypes.data,
                                                len(fractions), None if e is None else e.ctypes.data, None if c is None else c.ctypes.data,
                                                int(create)):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(st))


@pytest.fixture(scope="module")
def host():
    return SelectHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, seed, fractions):
    """sequences, a matrix, and NumPy's answers for the fractions"""
    from tests.synth import make_protein_set
    seqs = make_protein_set(n, 8, 20, seed)
    matrix = random_full(n, 400, seed)
    tri = np.sort(matrix[np.triu_indices(n, 1)])
    ranks = [python_rank(len(tri), q) for q in fractions]
    values = np.array([tri[r] for r in ranks], np.int32)
    below = np.searchsorted(tri, values, "left").astype(np.int64)
    return seqs, matrix, values, below


def assert_written(path, fractions, values, below, edge_min, cluster_min):
    m = len(fractions)
    got_q, got_v, got_b = h5_array(path, "score_quantiles", "<f8"), h5_array(path, "score_quantile_values", "<i4"), h5_array(path, "score_quantile_below", "<i8")
    assert got_q.tobytes() == np.asarray(fractions, "<f8").tobytes()  # the fractions as given, bit for bit
    assert np.array_equal(got_v, values) and np.array_equal(got_b, below)
    for name, kind in zip(QUANTILE_SETS, ("H5T_IEEE_F64LE", "H5T_STD_I32LE", "H5T_STD_I64LE")):
        props = h5_header(path, name)
        assert kind in props and f"( {m} )" in props and "CONTIGUOUS" in props, props
    for name, want in (("edge_min_score", edge_min), ("cluster_min_score", cluster_min)):
        if want is None:
            assert "/" + name not in h5_names(path)
        else:
            props = h5_header(path, "/" + name)
            assert "H5T_STD_I32LE" in props and "( 1 )" in props, props
            assert h5_array(path, name, "<i4").tolist() == [want]


@pytest.mark.parametrize("n,compression,fractions,cuts", [(40, 0, [0.99], (True, False)), (300, 0, [0.5, 0.0, 1.0, 0.5], (False, True)),
                                                          (300, 4, [k / 15 for k in range(16)], (True, True)), (40, 0, [0.25], (False, False))])
def test_quantiles_are_added_to_a_finished_file(n, compression, fractions, cuts, host, protein_lut, tmp_path):
    seqs, matrix, values, below = case(n, 5, fractions)
    edge_min = int(values[0]) if cuts[0] else None
    cluster_min = int(values[-1]) if cuts[1] else None
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, compression)
    shutil.copy(path, before)
    host.write_quantiles(path, seqs, protein_lut, fractions, values, below, edge_min, cluster_min, create=False)
    assert h5_names(path) == {"/sequences", "/similarity_matrix", *QUANTILE_SETS} | ({"/edge_min_score"} if cuts[0] else set()) | (
        {"/cluster_min_score"} if cuts[1] else set())
    assert_written(path, fractions, values, below, edge_min, cluster_min)
    for name in ("/similarity_matrix", "/sequences"):
        res = subprocess.run([str(H5DIFF), str(before), str(path), name], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(h5_matrix(path, n), matrix) and h5_sequences(path) == seqs


def test_create_only_has_sequences_and_no_matrix(host, protein_lut, tmp_path):
    fractions = [0.9, 0.1]
    seqs, _, values, below = case(50, 6, fractions)
    path = tmp_path / "only.h5"
    host.write_quantiles(path, seqs, protein_lut, fractions, values, below, int(values[0]), None, create=True)
    assert h5_names(path) == {"/sequences", *QUANTILE_SETS, "/edge_min_score"}
    assert h5_sequences(path) == seqs
    assert_written(path, fractions, values, below, int(values[0]), None)


def test_malformed_arrays_are_an_error_not_a_crash(host, protein_lut, tmp_path):
    fractions = [0.9, 0.1]
    seqs, _, values, below = case(50, 8, fractions)
    path = tmp_path / "bad.h5"
    pairs = 50 * 49 // 2
    for f, b, message in (([0.9, 1.5], below, "fraction"), ([float("nan"), 0.1], below, "fraction"), (fractions, [-1, 0], "pairs below"),
                          (fractions, [0, pairs], "pairs below"), ([0.5] * 17, [0] * 17, "1-16"), ([], [], "1-16")):
        with pytest.raises(HostError, match=message):
            host.write_quantiles(path, seqs, protein_lut, f, np.resize(values, len(f)), b, None, None, create=True)
        assert not path.exists()
    host.write_quantiles(path, seqs, protein_lut, fractions, values, below, None, None, create=True)  # ... and the library goes on working
    assert_written(path, fractions, values, below, None, None)


def test_appending_to_a_missing_file_is_an_error(host, protein_lut, tmp_path):
    seqs, _, values, below = case(20, 9, [0.5])
    with pytest.raises(HostError, match="Failed to open"):
        host.write_quantiles(tmp_path / "nothing.h5", seqs, protein_lut, [0.5], values, below, None, None, create=False)
    assert not (tmp_path / "nothing.h5").exists()


# ---- the tool's option errors ---------------------------------------------------------------------------------------------------
REFUSED = [
    (["--min-quantile", "x"], "Quantile must be a number between 0 and 1"),
    (["--min-quantile", "1.5"], "Quantile must be a number between 0 and 1"),
    (["--min-quantile", "nan"], "Quantile must be a number between 0 and 1"),
    (["--quantiles", "0.5,,0.7"], "Quantile must be a number between 0 and 1"),
    (["--clusters-quantile", "-0.1"], "Quantile must be a number between 0 and 1"),
    (["--min-score", "5", "--min-quantile", "0.9"], "--min-score and --min-quantile conflict"),
    (["--clusters", "5", "--clusters-quantile", "0.9"], "--clusters and --clusters-quantile conflict"),
    (["--quantiles", ",".join(["0.5"] * 17)], "At most 16 quantiles"),
    (["--min-quantile", "0.9", "--clusters-quantile", "0.9", "--quantiles", ",".join(["0.5"] * 15)], "At most 16 quantiles"),
    (["--linkage-only", "--min-quantile", "0.9"], "--linkage-only and --min-score conflict"),
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


def test_help_documents_the_three_options():
    cli = ROOT / "cli" / "seqalign"
    if not cli.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    text = subprocess.run([str(cli), "-h"], capture_output=True, text=True, timeout=120).stdout
    for word in ("--min-quantile Q", "--clusters-quantile Q", "--quantiles Q1,Q2", "/score_quantile_values", "/edge_min_score", "/cluster_min_score"):
        assert word in text, word
