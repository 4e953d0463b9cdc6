"""CPU: the host side of the alignments feature (include/seqalign_hip.h "alignments for chosen pairs", the tool's --alignments,
sa_host_write_alignments of cli/libsa_host.so) as far as it goes without a device: argument validation behind the ABI, the
no-device failure, the tool's refusal and help text, the writer's three datasets, and that the product library still does not
link the checker."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CLI = ROOT / "cli" / "seqalign"


@pytest.fixture(scope="module")
def small(sa):
    from tests.synth import make_protein_set
    return sa.SequenceStore.from_sequences(make_protein_set(12, 10, 40, 3)), sa.Scoring.from_names("ga", "blosum62", gap_open=10, gap_extend=1)


@pytest.mark.parametrize("pairs,message", [
    ([(3, 3)], "a == b"),
    ([(0, 1), (5, 5)], r"pair 1 = \(5, 5\)"),
    ([(0, 12)], "out of range"),
    ([(-1, 0)], "out of range"),
])
def test_bad_pair_lists_fail_with_a_message(pairs, message, sa, small):
    store, scoring = small
    with pytest.raises(sa.AlignError, match=message):
        sa.hip_alignments(store, scoring, pairs)


def test_negative_count_and_null_lists_fail_with_a_message(sa, small):
    store, scoring = small
    lib = sa.load_library()
    sc = scoring._as_c()
    a = np.zeros(4, np.int32)
    assert not lib.sa_hip_alignments(store._as_c(), C.byref(sc), a.ctypes.data, a.ctypes.data, -1)
    assert b"negative" in lib.sa_last_error()
    assert not lib.sa_hip_alignments(store._as_c(), C.byref(sc), None, None, 3)
    assert b"null pair list" in lib.sa_last_error()
    assert not lib.sa_ctx_alignments(None, a.ctypes.data, a.ctypes.data, 0)
    assert b"null context" in lib.sa_last_error()
    # the accessors take a null handle
    runs = C.c_int64(7)
    assert not lib.sa_alns_records(None) and not lib.sa_alns_cigar(None, C.byref(runs)) and runs.value == 0 and lib.sa_alns_count(None) == 0
    lib.sa_alns_destroy(None)


def test_no_device_fails_loudly(sa, small):
    if sa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    store, scoring = small
    with pytest.raises(sa.AlignError, match="No HIP devices"):
        sa.hip_alignments(store, scoring, [(0, 1), (4, 2)])
    with pytest.raises(sa.AlignError, match="No HIP devices"):
        sa.hip_alignments(store, scoring, [])   # even the empty list needs a device: there is no host path to fall back to
    assert sa.last_alignments_seconds() == 0.0


def test_record_layout_matches_the_header(sa):
    from sequencealigner_amd.binding import ALN_DTYPE
    text = (ROOT / "include" / "seqalign_hip.h").read_text()
    body = text[text.index("struct sa_aln {"):]
    body = body[:body.index("};")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(\w+)\s*[,;]", body)
    assert tuple(names) == ALN_DTYPE.names and ALN_DTYPE.itemsize == 40 and ALN_DTYPE.fields["cigar_off"][1] == 32


def test_cigar_string_and_aligned_strings(sa):
    from sequencealigner_amd.binding import ALN_DTYPE, Alignments
    store = sa.SequenceStore.from_sequences(["ARNDW", "ARW"])
    rec = np.zeros(2, ALN_DTYPE)
    rec[0] = (0, 0, 5, 0, 3, 5, 3, 3, 0)   # a = 0, b = 1: 2M 2I 1M
    rec[1] = (0, 0, 3, 0, 5, 5, 3, 3, 3)   # mirrored: 2M 2D 1M
    cigar = np.array([2 << 4 | 0, 2 << 4 | 1, 1 << 4 | 0, 2 << 4 | 0, 2 << 4 | 2, 1 << 4 | 0], np.uint32)
    alns = Alignments(pairs=np.array([[0, 1], [1, 0]], np.int32), records=rec, cigar=cigar)
    assert alns.cigar_string(0) == "2M2I1M" and alns.cigar_string(1) == "2M2D1M"
    assert alns.aligned(0, store) == ("ARNDW", "AR--W") and alns.aligned(1, store) == ("AR--W", "ARNDW")


def run_cli(*args):
    if not CLI.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    return subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=120)


def test_cli_refuses_alignments_without_k(tmp_path):
    fasta = tmp_path / "in.fasta"
    fasta.write_text(">a\nARND\n>b\nARNW\n>c\nWWWW\n")
    out = tmp_path / "out.h5"
    res = run_cli("-i", fasta, "-o", out, "-a", "nw", "-m", "blosum62", "-p", 4, "-F", "--alignments")
    assert res.returncode == 1 and "--alignments requires -k" in res.stderr and "usage information" in res.stderr, res.stderr
    assert not out.exists()


def test_cli_help_documents_the_option_and_the_ops():
    res = run_cli("-h")
    assert res.returncode == 0
    for needle in ("--alignments", "/neighbor_alignment_records", "/neighbor_cigar_offsets", "/neighbor_cigars", "0 = M", "1 = I", "2 = D"):
        assert needle in res.stdout, needle


def test_writer_adds_three_datasets(sa, tmp_path):
    from sequencealigner_amd.binding import ALN_DTYPE
    from tests.host_binding import H5DUMP, _Store
    from tests.test_neighbors_host import NeighborsHost, h5_dataset, h5_names
    from tests.synth import make_protein_set
    host = NeighborsHost()
    host.lib.sa_host_write_alignments.argtypes = [C.c_char_p, C.POINTER(_Store), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
    host.lib.sa_host_write_alignments.restype = C.c_int
    n, k = 30, 4
    rng = np.random.default_rng(4)
    seqs = make_protein_set(n, 8, 20, 9)
    lut = sa.Scoring.from_names("nw", "blosum62", gap_pen=4).lut
    index = rng.integers(0, n, size=(n, k), dtype=np.int32)
    score = rng.integers(-99, 99, size=(n, k), dtype=np.int32)
    path = tmp_path / "only.h5"
    host.write_neighbors(path, seqs, lut, k, index, score, create=True)
    rec = np.zeros(n * k, ALN_DTYPE)
    for f in ALN_DTYPE.names[:7]:
        rec[f] = rng.integers(-1000, 1000, n * k)
    rec["cigar_len"] = rng.integers(0, 4, n * k)   # zero-length CIGARs among them
    rec["cigar_off"] = np.concatenate([[0], np.cumsum(rec["cigar_len"])[:-1]])
    runs = int(rec["cigar_len"].sum())
    cigar = rng.integers(0, 2**32 - 1, runs, dtype=np.uint64).astype(np.uint32)

    def write(target, records, cig, count):
        st = host.parse(b"".join(b">s\n" + s + b"\n" for s in seqs), "fasta", lut)
        try:
            return host.lib.sa_host_write_alignments(str(target).encode(), C.byref(st), k, records.ctypes.data, cig.ctypes.data if count else None, count)
        finally:
            host.lib.sa_host_store_free(C.byref(st))

    assert write(path, rec, cigar, runs) == 0
    assert h5_names(path) == {"/sequences", "/neighbor_indices", "/neighbor_scores", "/neighbor_alignment_records",
                              "/neighbor_cigar_offsets", "/neighbor_cigars"}
    fields = h5_dataset(path, "neighbor_alignment_records", (n * k, 8))
    for col, f in enumerate(ALN_DTYPE.names[:8]):
        assert np.array_equal(fields[:, col], rec[f]), f

    def typed(name, dtype):
        out = path.with_name(name + ".bin")
        subprocess.check_call([str(H5DUMP), "-d", "/" + name, "-b", "LE", "-o", str(out), str(path)], stdout=subprocess.DEVNULL)
        return np.fromfile(out, dtype=dtype)

    offsets = typed("neighbor_cigar_offsets", "<i8")
    assert np.array_equal(offsets[:-1], rec["cigar_off"]) and offsets[-1] == runs and offsets.shape == (n * k + 1,)
    assert np.array_equal(typed("neighbor_cigars", "<u4"), cigar)
    assert np.array_equal(h5_dataset(path, "neighbor_indices", (n, k)), index)   # what was there stays
    props = subprocess.run([str(H5DUMP), "-p", "-H", str(path)], capture_output=True, text=True).stdout
    assert "H5T_STD_I64LE" in props and "H5T_STD_U32LE" in props and f"( {n}, {k}, 8 )" in props, props
    # a missing file is an error, not a crash; so is a second write into the same file
    assert write(tmp_path / "nothing.h5", rec, cigar, runs) == 1 and "Failed to open" in host._err()
    assert write(path, rec, cigar, runs) == 1


def test_product_library_still_does_not_link_the_oracle(sa):
    out = subprocess.run(["ldd", str(sa.library_path())], capture_output=True, text=True).stdout
    assert "oracle" not in out and "seqalign_ref" not in out
    for src in ("sa_traceback.hip", "sa_traceback_core.h"):
        assert "oracle" not in (ROOT / "sequencealigner_amd" / "csrc" / src).read_text()
