"""CPU: sa_host_write_edges of cli/libsa_host.so (the --min-score option's writer) through ctypes: /edge_offsets (N + 1 I64LE),
/edge_indices and /edge_scores (E I32LE), added to a finished file without touching what is in it, or written with /sequences
alone (--edges-only); and the tool's option errors, which need no device."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF, H5DUMP, ROOT, Host, HostError, _Store, h5_matrix, h5_sequences
from tests.test_neighbors_host import h5_names

EDGE_SETS = ("/edge_offsets", "/edge_indices", "/edge_scores")


class EdgesHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_edges.argtypes = [C.c_char_p, C.POINTER(_Store), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        self.lib.sa_host_write_edges.restype = C.c_int

    def write_edges(self, path, seqs, lut, offsets, index, score, create):
        st = self.parse(b"".join(b">s\n" + s + b"\n" for s in seqs), "fasta", lut)
        try:
            offsets = np.ascontiguousarray(offsets, np.int64)
            index = np.ascontiguousarray(index, np.int32)
            score = np.ascontiguousarray(score, np.int32)
            if self.lib.sa_host_write_edges(str(path).encode(), C.byref(st), offsets.ctypes.data, index.ctypes.data if index.size else None,
                                            score.ctypes.data if score.size else None, int(create)):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(st))


def h5_array(path, name: str, dtype: str) -> np.ndarray:
    """a 1-D dataset through h5dump -b LE (h5py is not installed); an extent of 0 leaves an empty or no file"""
    out = path.with_name(path.name + "." + name + ".bin")
    if out.exists():
        out.unlink()
    subprocess.check_call([str(H5DUMP), "-d", "/" + name, "-b", "LE", "-o", str(out), str(path)], stdout=subprocess.DEVNULL)
    return np.fromfile(out, dtype=dtype) if out.exists() else np.zeros(0, dtype)


def h5_edges(path, n: int):
    offsets = h5_array(path, "edge_offsets", "<i8")
    assert offsets.shape == (n + 1,)
    return offsets, h5_array(path, "edge_indices", "<i4"), h5_array(path, "edge_scores", "<i4")


def h5_header(path, name: str) -> str:
    return subprocess.run([str(H5DUMP), "-p", "-H", "-d", name, str(path)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def host():
    return EdgesHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, seed, density=0.1):
    """sequences, a symmetric matrix and a CSR of about `density` of its entries (the writer takes any well-formed CSR)"""
    from tests.synth import make_protein_set
    rng = np.random.default_rng(seed)
    seqs = make_protein_set(n, 8, 20, seed)
    matrix = rng.integers(-200, 200, size=(n, n), dtype=np.int32)
    matrix = np.triu(matrix, 1) + np.triu(matrix, 1).T
    a = rng.random((n, n)) < density
    np.fill_diagonal(a, False)
    offsets = np.concatenate([[0], np.cumsum(a.sum(1))]).astype(np.int64)
    index = np.nonzero(a)[1].astype(np.int32)
    score = rng.integers(-2**31, 2**31 - 1, size=index.size, dtype=np.int64).astype(np.int32)
    return seqs, matrix, offsets, index, score


def assert_types_and_extents(path, n, e):
    for name, kind, extent in (("/edge_offsets", "H5T_STD_I64LE", n + 1), ("/edge_indices", "H5T_STD_I32LE", e), ("/edge_scores", "H5T_STD_I32LE", e)):
        props = h5_header(path, name)
        assert kind in props and f"( {extent} )" in props, props
        if extent:
            assert "CONTIGUOUS" in props, props


@pytest.mark.parametrize("n,compression", [(40, 0), (300, 0), (300, 4)])
def test_edges_are_added_to_a_finished_file(n, compression, host, protein_lut, tmp_path):
    seqs, matrix, offsets, index, score = case(n, 5)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, compression)
    shutil.copy(path, before)
    host.write_edges(path, seqs, protein_lut, offsets, index, score, create=False)
    assert h5_names(path) == {"/sequences", "/similarity_matrix", *EDGE_SETS}
    got = h5_edges(path, n)
    assert np.array_equal(got[0], offsets) and np.array_equal(got[1], index) and np.array_equal(got[2], score)
    for name in ("/similarity_matrix", "/sequences"):
        res = subprocess.run([str(H5DIFF), str(before), str(path), name], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(h5_matrix(path, n), matrix) and h5_sequences(path) == seqs
    assert_types_and_extents(path, n, index.size)


def test_create_only_has_sequences_and_no_matrix(host, protein_lut, tmp_path):
    n = 50
    seqs, _, offsets, index, score = case(n, 6)
    path = tmp_path / "only.h5"
    host.write_edges(path, seqs, protein_lut, offsets, index, score, create=True)
    assert h5_names(path) == {"/sequences", *EDGE_SETS}
    assert h5_sequences(path) == seqs
    got = h5_edges(path, n)
    assert np.array_equal(got[0], offsets) and np.array_equal(got[1], index) and np.array_equal(got[2], score)
    assert_types_and_extents(path, n, index.size)


@pytest.mark.parametrize("create", [True, False])
def test_no_edge_at_all_still_writes_the_three_datasets(create, host, protein_lut, tmp_path):
    n = 30
    seqs, matrix, _, _, _ = case(n, 7)
    path = tmp_path / "empty.h5"
    if not create:
        host.write_hdf5(path, seqs, protein_lut, matrix, False, 0)
    host.write_edges(path, seqs, protein_lut, np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), create=create)
    assert set(EDGE_SETS) <= h5_names(path)
    offsets, index, score = h5_edges(path, n)
    assert not offsets.any() and index.shape == (0,) and score.shape == (0,)
    assert_types_and_extents(path, n, 0)


def test_malformed_arrays_are_an_error_not_a_crash(host, protein_lut, tmp_path):
    n = 50
    seqs, _, offsets, index, score = case(n, 8)
    path = tmp_path / "bad.h5"
    first = offsets.copy()
    first[0] = 1
    down = offsets.copy()
    down[n // 2] = down[n // 2 + 1] + 1  # (row n/2 - 1 grows past the end of row n/2: the next step decreases)
    low, high = index.copy(), index.copy()
    low[3], high[-1] = -1, n
    for off, idx, message in ((first, index, "start at 0"), (down, index, "decrease"), (offsets, low, "outside"), (offsets, high, "outside")):
        with pytest.raises(HostError, match=message):
            host.write_edges(path, seqs, protein_lut, off, idx, score, create=True)
        assert not path.exists()
    # ... and the library goes on working
    host.write_edges(path, seqs, protein_lut, offsets, index, score, create=True)
    assert np.array_equal(h5_edges(path, n)[1], index)


def test_appending_to_a_missing_file_is_an_error(host, protein_lut, tmp_path):
    seqs, _, offsets, index, score = case(20, 9)
    with pytest.raises(HostError, match="Failed to open"):
        host.write_edges(tmp_path / "nothing.h5", seqs, protein_lut, offsets, index, score, create=False)
    assert not (tmp_path / "nothing.h5").exists()


@pytest.mark.parametrize("bad,message", [
    (["--edges-only"], "--edges-only requires --min-score"),
    (["--min-score", "x"], "Minimum score must be an integer"),
    (["--min-score", "3000000000"], "Minimum score must be an integer"),
    (["--min-score", "5", "--edges-only", "-k", "5"], "--edges-only and -k, --neighbors conflict"),
])
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
