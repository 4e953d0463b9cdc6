"""CPU: the host-only side of percent identity through the binding (sa_pid_value against Python's integers; the argument checks
of the device calls that come before any device is looked for: null pointers, a denominator outside its enum, every output
null, each through sa_last_error with nothing written and followed by a call that works), sa_host_write_identity of
cli/libsa_host.so (the writer of --identity) through ctypes: /identity_rule (1 I32LE) and /identity_scale (1 I32LE), added to a
finished file without touching what is in it; and the tool's option errors, which need no device."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF, ROOT, Host, HostError, h5_matrix, h5_sequences
from tests.linkage_ref import random_full
from tests.test_edges_host import h5_array, h5_header
from tests.test_neighbors_host import h5_names

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
SCALE = 1000000
ID_SETS = ("/identity_rule", "/identity_scale")
POISON = -0x5A5A5A5B
COLUMNS, SHORTER, LONGER, MEAN = 0, 1, 2, 3


def python_pid(identities, columns, li, lj, denom):
    """the contract of include/seqalign_hip.h, with Python's integers"""
    den, num = {COLUMNS: (columns, identities * SCALE), SHORTER: (min(li, lj), identities * SCALE), LONGER: (max(li, lj), identities * SCALE),
                MEAN: (li + lj, 2 * identities * SCALE)}[denom]
    return INT32_MIN if den <= 0 else max(INT32_MIN, min(INT32_MAX, num // den))


# ---- the library's host-only calls ---------------------------------------------------------------------------------------------
def test_constants(sa):
    assert (sa.PID_COLUMNS, sa.PID_SHORTER, sa.PID_LONGER, sa.PID_MEAN) == (0, 1, 2, 3)
    assert sa.load_library().sa_abi_version() == 4  # additions only


def test_pid_value_is_pythons_floor_division(sa):
    lens = [1, 2, 3, 7, 64, 65, 1000, INT32_MAX // 2]
    checked = 0
    for denom in (COLUMNS, SHORTER, LONGER, MEAN):
        for li in lens:
            for lj in lens:
                for cols in (0, max(li, lj), min(li + lj, INT32_MAX)):
                    top = min(li, lj, cols)
                    for ident in {0, top, max(top - 1, 0), top // 2, top // 3}:
                        want = python_pid(ident, cols, li, lj, denom)
                        assert sa.pid_value(ident, cols, li, lj, denom) == want, (ident, cols, li, lj, denom)
                        assert want == INT32_MIN or 0 <= want <= SCALE
                        checked += 1
    assert checked > 2000
    assert sa.pid_value(1, 3, 5, 9, COLUMNS) == 333333 and sa.pid_value(2, 3, 5, 9, COLUMNS) == 666666  # floor, not rounding
    assert sa.pid_value(5, 9, 5, 9, SHORTER) == SCALE and sa.pid_value(5, 9, 5, 9, LONGER) == 555555 and sa.pid_value(5, 9, 5, 9, MEAN) == 714285
    assert sa.pid_value(0, 0, 5, 9, COLUMNS) == INT32_MIN and sa.pid_value(0, 0, 5, 9, SHORTER) == 0  # the empty SW alignment


@pytest.mark.parametrize("denom", [-1, 4, 17, INT32_MIN, INT32_MAX])
def test_pid_value_refuses_a_denominator_outside_the_enum(denom, sa):
    lib = sa.load_library()
    with pytest.raises(sa.AlignError, match=f"denom {denom} is none of"):
        sa.pid_value(5, 7, 7, 7, denom)
    assert lib.sa_pid_value(5, 7, 7, 7, denom) == INT32_MIN and b"sa_pid_value" in lib.sa_last_error()
    assert sa.pid_value(5, 7, 7, 7, COLUMNS) == 714285  # ... and the library goes on working
    with pytest.raises(sa.AlignError, match="int32"):
        sa.pid_value(2**31, 1, 1, 1, 0)


def small_case(sa):
    from tests.synth import make_protein_set
    return sa.SequenceStore.from_sequences(make_protein_set(5, 8, 12, 3)), sa.Scoring.from_names("nw", "blosum62", gap_pen=4)


ONE_CALLS = ["neighbors", "edges", "linkage", "select", "edges_at_rank", "linkage_with_ranks"]


def one_call(sa, which, store, scoring, pid):
    return {"neighbors": lambda: sa.hip_neighbors(store, scoring, 2, pid=pid),
            "edges": lambda: sa.hip_edges(store, scoring, 0, pid=pid),
            "linkage": lambda: sa.hip_linkage(store, scoring, pid=pid),
            "select": lambda: sa.hip_select(store, scoring, [0, 9], pid=pid),
            "edges_at_rank": lambda: sa.hip_edges_at_rank(store, scoring, 5, pid=pid),
            "linkage_with_ranks": lambda: sa.hip_linkage_with_ranks(store, scoring, [0, 9], pid=pid)}[which]()


@pytest.mark.parametrize("which", ONE_CALLS)
@pytest.mark.parametrize("denom", [4, -1])
def test_one_call_variants_refuse_a_bad_denominator_before_a_device_is_looked_for(which, denom, sa):
    store, scoring = small_case(sa)
    with pytest.raises(sa.AlignError, match=f"sa_hip_{which}_pid: denom {denom} is none of"):
        one_call(sa, which, store, scoring, denom)
    assert sa.pid_value(3, 4, 4, 4, MEAN) == 750000  # ... and the library goes on working


def test_bad_arguments_are_refused_with_nothing_written(sa):
    from sequencealigner_amd.binding import _IdentityOut
    lib = sa.load_library()
    store, scoring = small_case(sa)
    sc, inp = scoring._as_c(), store._as_c()
    out = np.full(64, POISON, np.int32)
    out64 = np.full(8, POISON, np.int64)
    ranks = np.zeros(1, np.int64)
    o, o64, r = out.ctypes.data, out64.ctypes.data, ranks.ctypes.data

    def refused(result, what="null"):
        assert not result and what.encode() in lib.sa_last_error(), lib.sa_last_error()
        assert sa.pid_value(1, 1, 1, 1, 0) == SCALE  # a valid call after every refusal

    good = _IdentityOut(None, o, None, None, 0)
    refused(lib.sa_ctx_identity_range(None, 0, 1, C.byref(good), None) == 0, "sa_ctx_identity_range: null argument")
    refused(lib.sa_zjob_identity(None, 0) == 0, "sa_zjob_identity: null argument")
    refused(lib.sa_hip_identity(inp, None, 0, o, o, o), "sa_hip_identity: null argument")
    refused(lib.sa_hip_identity(inp, C.byref(sc), 0, None, None, None), "sa_hip_identity: every output is null")
    refused(lib.sa_hip_identity(inp, C.byref(sc), 4, o, o, o), "sa_hip_identity: denom 4 is none of")
    refused(lib.sa_hip_identity(inp, C.byref(sc), -1, None, None, o), "sa_hip_identity: denom -1 is none of")
    refused(lib.sa_hip_neighbors_pid(inp, None, 2, o, o, 0))
    refused(lib.sa_hip_neighbors_pid(inp, C.byref(sc), 2, None, o, 0))
    refused(lib.sa_hip_neighbors_pid(inp, C.byref(sc), 2, o, None, 0))
    refused(lib.sa_hip_neighbors_pid(inp, C.byref(sc), 5, o, o, 0), "sa_hip_neighbors_pid: ")  # k > N - 1
    refused(lib.sa_hip_edges_pid(inp, None, 0, 0))
    refused(lib.sa_hip_linkage_pid(inp, None, 0))
    refused(lib.sa_hip_select_pid(inp, None, r, 1, o, o64, 0))
    refused(lib.sa_hip_select_pid(inp, C.byref(sc), None, 1, o, o64, 0))
    refused(lib.sa_hip_select_pid(inp, C.byref(sc), r, 1, None, o64, 0))
    refused(lib.sa_hip_select_pid(inp, C.byref(sc), r, 1, o, None, 0))
    bad_rank = np.array([10], np.int64)  # P = 10
    refused(lib.sa_hip_select_pid(inp, C.byref(sc), bad_rank.ctypes.data, 1, o, o64, 0), "sa_hip_select_pid: ")
    cut, below = C.c_int32(POISON), C.c_int64(POISON)
    refused(lib.sa_hip_edges_at_rank_pid(inp, None, 0, C.byref(cut), C.byref(below), 0))
    refused(lib.sa_hip_edges_at_rank_pid(inp, C.byref(sc), 0, None, C.byref(below), 0))
    refused(lib.sa_hip_linkage_with_ranks_pid(inp, None, r, 1, o, o64, 0))
    refused(lib.sa_hip_linkage_with_ranks_pid(inp, C.byref(sc), r, 1, None, o64, 0))
    # the messages name the entry point that was called
    assert not lib.sa_hip_edges_pid(inp, None, 0, 0) and b"sa_hip_edges_pid" in lib.sa_last_error()
    assert not lib.sa_hip_edges(inp, None, 0) and b"sa_hip_edges:" in lib.sa_last_error()
    assert (out == POISON).all() and (out64 == POISON).all() and cut.value == POISON and below.value == POISON


def test_the_binding_refuses_norm_and_pid_together(sa):
    store, scoring = small_case(sa)
    both = dict(norm=sa.Norm(), pid=0)
    for call in (lambda: sa.hip_neighbors(store, scoring, 2, **both), lambda: sa.hip_edges(store, scoring, 0, **both),
                 lambda: sa.hip_linkage(store, scoring, **both), lambda: sa.hip_select(store, scoring, [0], **both),
                 lambda: sa.hip_edges_at_rank(store, scoring, 0, **both), lambda: sa.hip_linkage_with_ranks(store, scoring, [0], **both)):
        with pytest.raises(sa.AlignError, match="norm and pid exclude each other"):
            call()
    with pytest.raises(sa.AlignError, match="int32"):
        sa.hip_linkage(store, scoring, pid=2**31)


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class IdentityHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_identity.argtypes = [C.c_char_p, C.c_int32]
        self.lib.sa_host_write_identity.restype = C.c_int

    def write_identity(self, path, denom):
        if self.lib.sa_host_write_identity(None if path is None else str(path).encode(), int(denom)):
            raise HostError(self._err())


@pytest.fixture(scope="module")
def host():
    return IdentityHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, seed):
    from tests.synth import make_protein_set
    return make_protein_set(n, 8, 20, seed), random_full(n, 400, seed)


def assert_written(path, denom):
    assert h5_array(path, "identity_rule", "<i4").tolist() == [denom]
    assert h5_array(path, "identity_scale", "<i4").tolist() == [SCALE]
    for name in ID_SETS:
        props = h5_header(path, name)
        assert "H5T_STD_I32LE" in props and "( 1 )" in props and "CONTIGUOUS" in props, props


@pytest.mark.parametrize("n,compression,denom", [(40, 0, 0), (300, 0, 3), (300, 4, 1)])
def test_datasets_are_added_to_a_finished_file(n, compression, denom, host, protein_lut, tmp_path):
    seqs, matrix = case(n, 5)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, compression)
    shutil.copy(path, before)
    host.write_identity(path, denom)
    assert h5_names(path) == {"/sequences", "/similarity_matrix", *ID_SETS}
    assert_written(path, denom)
    for name in ("/similarity_matrix", "/sequences"):
        res = subprocess.run([str(H5DIFF), str(before), str(path), name], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(h5_matrix(path, n), matrix) and h5_sequences(path) == seqs


def test_bad_arguments_are_an_error_and_touch_nothing(host, protein_lut, tmp_path):
    seqs, matrix = case(30, 8)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, 0)
    shutil.copy(path, before)
    for p, denom, message in ((None, 0, "missing"), (path, 4, "denominator 4"), (path, -1, "denominator -1")):
        with pytest.raises(HostError, match=message):
            host.write_identity(p, denom)
        assert path.read_bytes() == before.read_bytes()
    host.write_identity(path, 2)  # ... and the library goes on working
    assert_written(path, 2)


def test_appending_to_a_missing_file_is_an_error(host, tmp_path):
    with pytest.raises(HostError, match="Failed to open"):
        host.write_identity(tmp_path / "nothing.h5", 0)
    assert not (tmp_path / "nothing.h5").exists()


# ---- the tool's option errors ---------------------------------------------------------------------------------------------------
REFUSED = [
    (["--identity", "columns"], "--identity requires something selected from the scores"),
    (["--identity", "mean", "--alignments"], "--alignments requires -k"),
    (["--identity", "column", "-k", "2"], "Identity denominator must be one of columns, shorter, longer, mean"),
    (["--identity", "COLUMNS", "-k", "2"], "Identity denominator must be one of columns"),
    (["--identity", "", "-k", "2"], "Identity denominator must be one of columns"),
    (["--identity", "self-min", "--linkage"], "Identity denominator must be one of columns"),
    (["--identity", "shorter", "--normalize", "len-min", "-k", "2"], "--identity and --normalize conflict"),
    (["--normalize", "self-min", "--linkage", "--identity=longer"], "--identity and --normalize conflict"),
    (["-k", "2", "--identity"], "--identity requires a parameter"),
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
    for word in ("--identity DENOM", "columns | shorter | longer | mean", "STAYS RAW", "/identity_rule", "/identity_scale", "parts per million",
                 "Not together", "--normalize"):
        assert word in text, word
