"""CPU: sa_host_write_neighbors of cli/libsa_host.so (the -k option's writer) through ctypes: /neighbor_indices and
/neighbor_scores, N x k I32LE, added to a finished file without touching what is in it, or written with /sequences alone
(--neighbors-only)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF, H5DUMP, Host, HostError, _Store, h5_matrix, h5_sequences


class NeighborsHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_neighbors.argtypes = [C.c_char_p, C.POINTER(_Store), C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
        self.lib.sa_host_write_neighbors.restype = C.c_int

    def write_neighbors(self, path, seqs, lut, k, index, score, create):
        st = self.parse(b"".join(b">s\n" + s + b"\n" for s in seqs), "fasta", lut)
        try:
            index = np.ascontiguousarray(index, np.int32)
            score = np.ascontiguousarray(score, np.int32)
            if self.lib.sa_host_write_neighbors(str(path).encode(), C.byref(st), int(k), index.ctypes.data, score.ctypes.data, int(create)):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(st))


def h5_dataset(path, name: str, shape) -> np.ndarray:
    out = path.with_name(path.name + "." + name + ".bin")
    subprocess.check_call([str(H5DUMP), "-d", "/" + name, "-b", "LE", "-o", str(out), str(path)], stdout=subprocess.DEVNULL)
    return np.fromfile(out, dtype="<i4").reshape(shape)


def h5_names(path) -> set:
    txt = subprocess.run([str(H5DUMP), "-n", str(path)], capture_output=True, text=True, check=True).stdout
    return {line.split()[1] for line in txt.splitlines() if line.strip().startswith("dataset")}


@pytest.fixture(scope="module")
def host():
    return NeighborsHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, k, seed):
    from tests.synth import make_protein_set
    rng = np.random.default_rng(seed)
    seqs = make_protein_set(n, 8, 20, seed)
    matrix = rng.integers(-200, 200, size=(n, n), dtype=np.int32)
    matrix = np.triu(matrix, 1) + np.triu(matrix, 1).T
    index = rng.integers(0, n, size=(n, k), dtype=np.int32)
    score = rng.integers(-2**31, 2**31 - 1, size=(n, k), dtype=np.int64).astype(np.int32)
    return seqs, matrix, index, score


@pytest.mark.parametrize("n,k,compression", [(40, 7, 0), (300, 64, 0), (300, 1, 4)])
def test_neighbors_are_added_to_a_finished_file(n, k, compression, host, protein_lut, tmp_path):
    seqs, matrix, index, score = case(n, k, 5)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, compression)
    shutil.copy(path, before)
    host.write_neighbors(path, seqs, protein_lut, k, index, score, create=False)
    assert h5_names(path) == {"/sequences", "/similarity_matrix", "/neighbor_indices", "/neighbor_scores"}
    assert np.array_equal(h5_dataset(path, "neighbor_indices", (n, k)), index)
    assert np.array_equal(h5_dataset(path, "neighbor_scores", (n, k)), score)
    for name in ("/similarity_matrix", "/sequences"):
        res = subprocess.run([str(H5DIFF), str(before), str(path), name], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(h5_matrix(path, n), matrix) and h5_sequences(path) == seqs
    props = subprocess.run([str(H5DUMP), "-p", "-H", "-d", "/neighbor_indices", str(path)], capture_output=True, text=True).stdout
    assert "H5T_STD_I32LE" in props and "CONTIGUOUS" in props and f"( {n}, {k} )" in props, props


def test_create_only_has_sequences_and_no_matrix(host, protein_lut, tmp_path):
    n, k = 50, 10
    seqs, _, index, score = case(n, k, 6)
    path = tmp_path / "only.h5"
    host.write_neighbors(path, seqs, protein_lut, k, index, score, create=True)
    assert h5_names(path) == {"/sequences", "/neighbor_indices", "/neighbor_scores"}
    assert h5_sequences(path) == seqs
    assert np.array_equal(h5_dataset(path, "neighbor_indices", (n, k)), index)
    assert np.array_equal(h5_dataset(path, "neighbor_scores", (n, k)), score)


@pytest.mark.parametrize("k", [0, -1, 65, 50, 2**31 - 1])
def test_bad_k_is_an_error_not_a_crash(k, host, protein_lut, tmp_path):
    n = 50  # k = 50 = N: one more than there are other sequences
    seqs, _, index, score = case(n, 64, 7)
    path = tmp_path / "bad.h5"
    with pytest.raises(HostError, match="Neighbor count"):
        host.write_neighbors(path, seqs, protein_lut, k, index, score, create=True)
    assert not path.exists()
    # ... and the library goes on working
    host.write_neighbors(path, seqs, protein_lut, 3, index[:, :3], score[:, :3], create=True)
    assert np.array_equal(h5_dataset(path, "neighbor_indices", (n, 3)), index[:, :3])


def test_appending_to_a_missing_file_is_an_error(host, protein_lut, tmp_path):
    seqs, _, index, score = case(20, 4, 8)
    with pytest.raises(HostError, match="Failed to open"):
        host.write_neighbors(tmp_path / "nothing.h5", seqs, protein_lut, 4, index, score, create=False)
