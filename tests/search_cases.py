"""What the search tests share (tests/test_search_host.py, tests/test_gpu_search.py, tests/test_gpu_search_cli.py): the query
lengths of the mixed-column store and the expectation of a search, which never comes from the code under test: the rectangle
is rows N.., columns ..N of the oracle's full matrix of db followed by queries, the hits np.lexsort((d, -scores))[:k] per row."""
import numpy as np

from tests.golden_util import tri_to_full

# 8-lane, 16-lane, s32 and strip-mined columns in one store (two of them twice)
MIXED_QUERY_LENGTHS = (5, 64, 65, 128, 129, 300, 700, 1024, 1025, 1500, 65, 1025)


def h5_strings(path, name: str) -> list:
    """a dataset of variable-length strings, /sequences or /query_sequences, through h5dump (h5py is not installed)"""
    import re
    import subprocess

    from tests.host_binding import H5DUMP
    txt = subprocess.run([str(H5DUMP), "-d", "/" + name, "-y", "-w", "0", str(path)], capture_output=True, text=True, check=True).stdout
    return [m.encode() for m in re.findall(r'"([^"]*)"', txt[txt.index("DATA {") + 6:])]


def expected_hits(rect: np.ndarray, k: int):
    m, n = rect.shape
    index, score = np.empty((m, k), np.int32), np.empty((m, k), np.int32)
    d = np.arange(n)
    for q in range(m):
        order = np.lexsort((d, -rect[q].astype(np.int64)))[:k]
        index[q], score[q] = order, rect[q, order]
    return index, score


def oracle_rect(sa, oracle, db_seqs, query_seqs, scoring):
    """rows N.., columns ..N of the oracle's full matrix of db followed by queries"""
    n = len(db_seqs)
    cat = sa.SequenceStore.from_sequences(list(db_seqs) + list(query_seqs))
    full = tri_to_full(oracle.align(cat, scoring, triangular=True), cat.num)
    return np.ascontiguousarray(full[n:, :n]).astype(np.int32)
