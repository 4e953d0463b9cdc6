"""CPU: the host-only readers of a single-linkage tree through the binding (sa_linkage_labels, sa_linkage_merges,
sa_linkage_scratch_bytes: validation, errors through sa_last_error with nothing written), sa_host_write_linkage of
cli/libsa_host.so (the --linkage option's writer) through ctypes: /linkage_pairs ((N - 1) x 2 I32LE), /linkage_scores (N - 1
I32LE) and /cluster_labels (N I32LE), added to a finished file without touching what is in it, or written with /sequences alone
(--linkage-only); and the tool's option errors, which need no device."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests.host_binding import H5DIFF, ROOT, Host, HostError, _Store, h5_matrix, h5_sequences
from tests.linkage_ref import kruskal_tree, labels_at, prim_tree, random_full
from tests.test_edges_host import h5_array, h5_header
from tests.test_neighbors_host import h5_dataset, h5_names

TREE_SETS = ("/linkage_pairs", "/linkage_scores")
POISON = -0x5A5A5A5B


# ---- the library's host-only calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,spread", [(2, 1), (17, 3), (130, 1000), (300, 5)])
def test_labels_and_merges_of_a_reference_tree(n, spread, sa):
    full = random_full(n, spread, 7 * n + spread)
    pairs, score = prim_tree(full)
    for t in sorted({int(score.min()) - 1, int(score.min()), int(np.median(score)), int(score.max()), int(score.max()) + 1, -2**31, 2**31 - 1}):
        want, want_clusters = labels_at(full, t)
        labels, clusters = sa.linkage_labels(pairs, score, n, t)
        assert labels.dtype == np.int32 and labels.shape == (n,) and clusters == want_clusters and np.array_equal(labels, want), t
    merges = sa.linkage_merges(pairs, n)
    assert merges.dtype == np.int32 and merges.shape == (n - 1, 3)
    # the convention of scipy.cluster.hierarchy, replayed: ids below N are sequences, N + u is what merge u made
    member = {v: {v} for v in range(n)}
    ident = list(range(n))
    for t, ((lo, hi), (left, right, size)) in enumerate(zip(pairs.tolist(), merges.tolist())):
        a, b = ident[lo], ident[hi]
        assert (left, right, size) == (min(a, b), max(a, b), len(member[a]) + len(member[b]))
        member[n + t] = member.pop(a) | member.pop(b)
        for v in member[n + t]:
            ident[v] = n + t
    assert len(member) == 1


def test_one_sequence_is_one_cluster(sa):
    labels, clusters = sa.linkage_labels(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 1, 0)
    assert labels.tolist() == [0] and clusters == 1
    assert sa.linkage_merges(np.zeros((0, 2), np.int32), 1).shape == (0, 3)


GOOD_PAIRS, GOOD_SCORE = [[0, 1], [2, 3], [1, 2], [3, 4]], [9, 9, 4, -3]


@pytest.mark.parametrize("pairs,score,message,merges_too", [
    ([[0, 1], [1, 2], [0, 2], [3, 4]], [9, 8, 7, 6], "cycle", True),
    ([[1, 0], [2, 3], [1, 2], [3, 4]], GOOD_SCORE, "lo < hi", True),
    ([[0, 1], [2, 2], [1, 2], [3, 4]], GOOD_SCORE, "lo < hi", True),
    ([[0, 1], [2, 3], [1, 2], [3, 5]], GOOD_SCORE, "out of range", True),
    ([[0, 1], [-1, 3], [1, 2], [3, 4]], GOOD_SCORE, "out of range", True),
    (GOOD_PAIRS, [9, 9, 4, 5], "order", False),
    ([[2, 3], [0, 1], [1, 2], [3, 4]], GOOD_SCORE, "order", False),
])
def test_trees_that_are_none_fail_with_nothing_written(pairs, score, message, merges_too, sa):
    lib = sa.load_library()
    n = 5
    p, s = np.array(pairs, np.int32), np.array(score, np.int32)
    out = np.full((4, n), POISON, np.int32)
    with pytest.raises(sa.AlignError, match=message):
        sa.linkage_labels(p, s, n, 0)
    assert lib.sa_linkage_labels(p.ctypes.data, s.ctypes.data, n, 0, out[0].ctypes.data) < 0
    if merges_too:
        with pytest.raises(sa.AlignError, match=message):
            sa.linkage_merges(p, n)
        assert lib.sa_linkage_merges(p.ctypes.data, n, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data) != 0
    assert (out == POISON).all()
    # ... and the process goes on working
    labels, clusters = sa.linkage_labels(GOOD_PAIRS, GOOD_SCORE, n, 5)
    assert labels.tolist() == [0, 0, 2, 2, 4] and clusters == 3
    assert sa.linkage_merges(GOOD_PAIRS, n).tolist() == [[0, 1, 2], [2, 3, 2], [5, 6, 4], [4, 7, 5]]


def test_null_arguments_and_bad_sizes(sa):
    lib = sa.load_library()
    p, s = np.array(GOOD_PAIRS, np.int32), np.array(GOOD_SCORE, np.int32)
    out = np.full((3, 5), POISON, np.int32)
    o = [row.ctypes.data for row in out]
    for args in ((None, s.ctypes.data, 5, 0, o[0]), (p.ctypes.data, None, 5, 0, o[0]), (p.ctypes.data, s.ctypes.data, 5, 0, None)):
        assert lib.sa_linkage_labels(*args) < 0 and b"null" in lib.sa_last_error()
    for args in ((None, 5, *o), (p.ctypes.data, 5, None, o[1], o[2]), (p.ctypes.data, 5, o[0], None, o[2]), (p.ctypes.data, 5, o[0], o[1], None)):
        assert lib.sa_linkage_merges(*args) != 0 and b"null" in lib.sa_last_error()
    assert lib.sa_linkage_labels(p.ctypes.data, s.ctypes.data, 0, 0, o[0]) < 0 and lib.sa_linkage_merges(p.ctypes.data, -3, *o) != 0
    assert (out == POISON).all()
    with pytest.raises(sa.AlignError, match="elements"):
        sa.linkage_labels(p[:3], s, 5, 0)
    with pytest.raises(sa.AlignError, match="elements"):
        sa.linkage_labels(p, s[:3], 5, 0)
    with pytest.raises(sa.AlignError, match="int32"):
        sa.linkage_labels(p, s, 5, 2**31)
    assert sa.linkage_scratch_bytes(0) == 0 and sa.linkage_scratch_bytes(-5) == 0
    sizes = [sa.linkage_scratch_bytes(n) for n in (1, 2, 65, 700, 100000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(b % 4 == 0 for b in sizes) and sizes[-1] < 64 * 100000


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class LinkageHost(Host):
    """the suite's host binding plus the one new entry point"""

    def __init__(self):
        super().__init__()
        self.lib.sa_host_write_linkage.argtypes = [C.c_char_p, C.POINTER(_Store), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        self.lib.sa_host_write_linkage.restype = C.c_int

    def write_linkage(self, path, seqs, lut, pairs, score, labels, create):
        st = self.parse(b"".join(b">s\n" + s + b"\n" for s in seqs), "fasta", lut)
        try:
            pairs = np.ascontiguousarray(pairs, np.int32)
            score = np.ascontiguousarray(score, np.int32)
            labels = None if labels is None else np.ascontiguousarray(labels, np.int32)
            if self.lib.sa_host_write_linkage(str(path).encode(), C.byref(st), pairs.ctypes.data if pairs.size else None,
                                              score.ctypes.data if score.size else None, None if labels is None else labels.ctypes.data,
                                              int(create)):
                raise HostError(self._err())
        finally:
            self.lib.sa_host_store_free(C.byref(st))


def h5_linkage(path, n: int):
    """(pairs (N - 1, 2), score (N - 1,)) as written"""
    return h5_dataset(path, "linkage_pairs", (n - 1, 2)), h5_array(path, "linkage_scores", "<i4")


@pytest.fixture(scope="module")
def host():
    return LinkageHost()


@pytest.fixture(scope="module")
def protein_lut(sa):
    return sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut


def case(n, seed):
    from tests.synth import make_protein_set
    seqs = make_protein_set(n, 8, 20, seed)
    matrix = random_full(n, 400, seed)
    pairs, score = kruskal_tree(matrix) if n <= 60 else prim_tree(matrix)
    labels, _ = labels_at(matrix, int(np.median(score)))
    return seqs, matrix, pairs, score, labels


def assert_types_and_extents(path, n, with_labels):
    for name, extent in (("/linkage_pairs", f"( {n - 1}, 2 )"), ("/linkage_scores", f"( {n - 1} )")) + ((("/cluster_labels", f"( {n} )"),) if with_labels else ()):
        props = h5_header(path, name)
        assert "H5T_STD_I32LE" in props and extent in props and "CONTIGUOUS" in props, props


@pytest.mark.parametrize("n,compression,with_labels", [(40, 0, False), (300, 0, True), (300, 4, False)])
def test_tree_is_added_to_a_finished_file(n, compression, with_labels, host, protein_lut, tmp_path):
    seqs, matrix, pairs, score, labels = case(n, 5)
    path, before = tmp_path / "out.h5", tmp_path / "before.h5"
    host.write_hdf5(path, seqs, protein_lut, matrix, False, compression)
    shutil.copy(path, before)
    host.write_linkage(path, seqs, protein_lut, pairs, score, labels if with_labels else None, create=False)
    assert h5_names(path) == {"/sequences", "/similarity_matrix", *TREE_SETS} | ({"/cluster_labels"} if with_labels else set())
    got = h5_linkage(path, n)
    assert np.array_equal(got[0], pairs) and np.array_equal(got[1], score)
    if with_labels:
        assert np.array_equal(h5_array(path, "cluster_labels", "<i4"), labels)
    for name in ("/similarity_matrix", "/sequences"):
        res = subprocess.run([str(H5DIFF), str(before), str(path), name], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(h5_matrix(path, n), matrix) and h5_sequences(path) == seqs
    assert_types_and_extents(path, n, with_labels)


@pytest.mark.parametrize("with_labels", [False, True])
def test_create_only_has_sequences_and_no_matrix(with_labels, host, protein_lut, tmp_path):
    n = 50
    seqs, _, pairs, score, labels = case(n, 6)
    path = tmp_path / "only.h5"
    host.write_linkage(path, seqs, protein_lut, pairs, score, labels if with_labels else None, create=True)
    assert h5_names(path) == {"/sequences", *TREE_SETS} | ({"/cluster_labels"} if with_labels else set())
    assert h5_sequences(path) == seqs
    got = h5_linkage(path, n)
    assert np.array_equal(got[0], pairs) and np.array_equal(got[1], score)
    assert_types_and_extents(path, n, with_labels)


def test_malformed_arrays_are_an_error_not_a_crash(host, protein_lut, tmp_path):
    n = 50
    seqs, _, pairs, score, labels = case(n, 8)
    path = tmp_path / "bad.h5"
    low, high, turned, above = pairs.copy(), pairs.copy(), pairs.copy(), labels.copy()
    low[3, 0], high[-1, 1], turned[7] = -1, n, turned[7, ::-1]
    above[4] = 5
    for p, lab, message in ((low, None, "outside"), (high, None, "outside"), (turned, None, "lo < hi"), (pairs, above, "smallest index")):
        with pytest.raises(HostError, match=message):
            host.write_linkage(path, seqs, protein_lut, p, score, lab, create=True)
        assert not path.exists()
    host.write_linkage(path, seqs, protein_lut, pairs, score, labels, create=True)  # ... and the library goes on working
    assert np.array_equal(h5_linkage(path, n)[0], pairs)


def test_appending_to_a_missing_file_is_an_error(host, protein_lut, tmp_path):
    seqs, _, pairs, score, _ = case(20, 9)
    with pytest.raises(HostError, match="Failed to open"):
        host.write_linkage(tmp_path / "nothing.h5", seqs, protein_lut, pairs, score, None, create=False)
    assert not (tmp_path / "nothing.h5").exists()


# ---- the tool's option errors ---------------------------------------------------------------------------------------------------
REFUSED = [
    (["--linkage-only", "-k", "5"], "--linkage-only and -k, --neighbors conflict"),
    (["--linkage-only", "--min-score", "5"], "--linkage-only and --min-score conflict"),
    (["--clusters", "x"], "Cluster score must be an integer"),
    (["--clusters", "3000000000"], "Cluster score must be an integer"),
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
