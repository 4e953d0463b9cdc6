"""GPU (-m gpu): the identity sweep (sa_k_identity, csrc/sa_identity.hip) on column sequences of 3 to 6 strips of 64 columns,
exactly, on the inputs that pin the decision-recording kernels there (tests/test_gpu_traceback_strips.py).

tests/test_gpu_identity.py checks sa_k_identity against the Python restatement up to 300 residues, over the alphabet ARN, under
default gaps and gaps of zero.  The kernel restates the sweep of sa_k_trace_fill on its own and adds what no other kernel has:
payloads (identities, columns) that travel through DPP beside their scores, a second boundary buffer (bndPM / bndPX) for the
payloads of a strip's last column, and for SW the end cell's payload reduced over lanes with the end key.  A payload taken from
the wrong neighbour on a tie in strip 3 leaves the right score and plausible identities and columns.  Here the stores of the
traceback file -- four-letter DNA at the strip edges, a long row against a short multi-strip column, the repeats, the two
planted Smith-Waterman pairs; imported, not copied -- go through sa_ctx_identity_range: one context and one call over the whole
triangle per scoring and denominator, all four outputs.  Scores are the oracle's for every pair of the triangle; identities
and columns are those of tests/traceback_ref.py for the case's pairs (lo the row sequence), pid is Python's //.  Every
comparison is exact; a second call gives the same bytes.

Sensitivity, from the reference alone (asserted on the CPU before the device is asked): the unordered pairs whose (identities,
columns) change when traceback_ref walks the same tables with the other order among equally good moves.  Nearly every change
is in the columns, not the identities.  Counts of these inputs (pairs that differ / pairs):

    nw dnafull gap 2 ............ 22 / 28        nw blosum62 gap 0 ........... 21 / 38
    ga dnafull 3 / 1 ............ 14 / 28        ga blosum62 3 / 1 ........... 14 / 38
    sw nuc44 3 / 1 .............. 19 / 28        sw blosum62 3 / 1 ........... 10 / 38
    ga dnafull 0 / 0 ............  0 / 28
    sw dnafull 4 / 4 ............  1 / 28
    ga dnafull 3 / 7 ............  0 / 28

The first three DNA scorings must reach 12 of 28, a protein scoring whose count is at least 8 half of it (FLOORS).  Nothing is
asserted for the other three DNA scorings: under them both walks end with the same counts, so they pin the sweep and the
boundary payloads -- a payload from the wrong strip, line or lane is still a wrong number -- not the tie order.

The SW end cell: `crossed` has equal maxima in strips 0 and 2 and the contract's end cell (smallest row) is not in the lowest
strip that holds one; `doubled` has four maxima in two strips.  Both are asserted on the reference's M, as the traceback file
does; the device's (identities, columns) must then be the reference's, which a lane reduction that carries the right key with
another lane's payload cannot give.

One more store: 12 DNA sequences of 130 to 320 residues with IUPAC ambiguity codes under dnafull, the whole triangle of 66
pairs against traceback_ref.  Under that table an ambiguity code scores as a match against the letters it stands for (A
against R: +1) without being equal to them: the contract counts equal codes, and the case asserts on the reference's
alignments that columns of the two kinds exist."""
import numpy as np
import pytest

from tests import traceback_ref
from tests.synth import make_dna_set
from tests.test_gpu_identity import COLUMNS, DENOMS, OUTPUTS, check_all, device_identity, packed_pairs, python_pid
from tests.test_gpu_identity import reference as triangle_reference
from tests.test_gpu_traceback_strips import DNA_SCORINGS, PROTEIN_SCORINGS, dna_case, maxima, protein_case, reference, scoring_id, strip_of

pytestmark = pytest.mark.gpu

# the least number of unordered pairs whose (identities, columns) the other tie order must change: 12 of 28 where the
# counts are 22, 14 and 19; half the measured count (docstring) for a protein scoring that reaches 8
FLOORS = {("dna", "nw", "dnafull", 2): 12, ("dna", "ga", "dnafull", 3, 1): 12, ("dna", "sw", "nuc44", 3, 1): 12,
          ("protein", "nw", "blosum62", 0): 10, ("protein", "ga", "blosum62", 3, 1): 7, ("protein", "sw", "blosum62", 3, 1): 5}

CASES = [pytest.param("dna", *s, id="dna-" + "-".join(map(scoring_id, s))) for s in DNA_SCORINGS] + \
        [pytest.param("protein", *s, id="protein-" + "-".join(map(scoring_id, s))) for s in PROTEIN_SCORINGS]


def floor_key(kind, method, matrix, gaps):
    return (kind, method, matrix) + tuple(v for v in gaps.values() if v is not False)


@pytest.mark.parametrize("kind,method,matrix,gaps", CASES)
def test_identity_beyond_the_second_strip_equals_the_python_restatement(kind, method, matrix, gaps, sa, oracle):
    seqs, unordered, planted = dna_case() if kind == "dna" else protein_case()
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    assert scoring.method == {"nw": 0, "ga": 1, "sw": 2}[method]
    lens = [len(s) for s in seqs]
    n = len(seqs)
    assert (n, len(unordered)) == ((22, 28) if kind == "dna" else (27, 38)) and len(set(unordered)) == len(unordered)
    assert all(lo < hi and 3 <= (lens[hi] + 63) // 64 <= 6 or (lens[lo], lens[hi]) == (320, 65) for lo, hi in unordered)   # 3 to 6 strips

    # ---- on the CPU, from the reference alone ----
    want, other, M = reference(scoring, seqs, unordered)
    sensitive = sum((want[p]["identities"], want[p]["columns"]) != (other[p]["identities"], other[p]["columns"]) for p in unordered)
    only_columns = sum(want[p]["identities"] == other[p]["identities"] and want[p]["columns"] != other[p]["columns"] for p in unordered)
    print(f"{kind} {method} {matrix} {gaps}: the other tie order changes (identities, columns) of {sensitive} of {len(unordered)} pairs "
          f"({only_columns} of them in the columns alone)")
    floor = FLOORS.get(floor_key(kind, method, matrix, gaps), 0)
    assert sensitive >= floor, f"only {sensitive} of {len(unordered)} pairs depend on the tie order, the case wants {floor}"
    if method == "sw" and planted:
        best, cells = maxima(M[planted["crossed"]])
        strips = {strip_of(cell) for cell in cells}
        assert best > 0 and len(strips) >= 2 and strip_of(min(cells)) > min(strips), (best, cells)   # (min: smallest r, then smallest c)
        end = want[planted["crossed"]]
        assert (end["a_end"], end["b_end"]) == min(cells) and end["columns"] > 0
        best, cells = maxima(M[planted["doubled"]])
        assert len(cells) >= 4 and len({strip_of(cell) for cell in cells}) >= 2 and len({r for r, _ in cells}) >= 2, (best, cells)

    # ---- the device: the whole triangle in one call per denominator ----
    store = sa.SequenceStore.from_sequences(seqs)
    triangle = packed_pairs(n)
    count = len(triangle)
    assert count == store.pairs == n * (n - 1) // 2
    scores = oracle.align(store, scoring, triangular=True)
    at = np.array([hi * (hi - 1) // 2 + lo for lo, hi in unordered], np.int64)
    assert all(triangle[k] == p for k, p in zip(at.tolist(), unordered))
    assert np.array_equal(scores[at], [want[p]["score"] for p in unordered])   # the restatement's scores are the oracle's
    ident = np.array([want[p]["identities"] for p in unordered], np.int32)
    cols = np.array([want[p]["columns"] for p in unordered], np.int32)
    with sa.Context(store, scoring, 0) as ctx:
        for denom in DENOMS:
            got = device_identity(ctx, 0, count, denom)
            again = device_identity(ctx, 0, count, denom)
            what = f"{kind} {method} {matrix} {gaps} denom {denom}"
            bad = np.flatnonzero(got["score"] != scores)
            assert bad.size == 0, f"{what}: {bad.size} of {count} scores differ from the oracle's, first: pair {triangle[bad[0]]}: {got['score'][bad[0]]} / {scores[bad[0]]}"
            for t, (lo, hi) in enumerate(unordered):
                k = int(at[t])
                have = {name: int(got[name][k]) for name in OUTPUTS}
                ref = dict(score=want[lo, hi]["score"], identities=int(ident[t]), columns=int(cols[t]),
                           pid=python_pid(int(ident[t]), int(cols[t]), lens[lo], lens[hi], denom))
                name = next((key for key, p in planted.items() if p == (lo, hi)), "")
                assert have == ref, (f"{what}: pair ({lo}, {hi}) {name}, rows {lens[lo]} x columns {lens[hi]} ({(lens[hi] + 63) // 64} strips):\n got  {have}\n want {ref}\n"
                                     f" other tie order: identities {other[lo, hi]['identities']}, columns {other[lo, hi]['columns']}")
            assert all(again[name].tobytes() == got[name].tobytes() for name in OUTPUTS), f"{what}: a second call gives other bytes"


IUPAC_SCORINGS = [("nw", dict(gap_pen=8)), ("ga", dict(gap_open=16, gap_extend=4))]   # those of test_dna_anchored_at_the_oracle


def kinds_of_columns(scoring, lo_seq, hi_seq, ref):
    """(equal, scored as a match without being equal) among the M columns of the reference's alignment of a pair lo < hi"""
    r, c, equal, alike = ref["a_begin"], ref["b_begin"], 0, 0
    for length, op in ref["cigar"]:
        if op == "M":
            for k in range(length):
                a, b = int(scoring.lut[lo_seq[r + k]]), int(scoring.lut[hi_seq[c + k]])
                equal += a == b
                alike += a != b and traceback_ref._sim(scoring, a, b) > 0
        r, c = r + (length if op != "D" else 0), c + (length if op != "I" else 0)
    assert (r, c) == (ref["a_end"], ref["b_end"]) and equal == ref["identities"]
    return equal, alike


@pytest.mark.parametrize("method,gaps", IUPAC_SCORINGS, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_ambiguity_codes_count_as_identities_only_when_equal(method, gaps, sa, oracle):
    seqs = make_dna_set(12, 130, 320, 6, iupac=True)
    lens = [len(s) for s in seqs]
    assert min(lens) >= 130 and max(lens) <= 320 and len({(n + 63) // 64 for n in lens}) >= 3 and any(set(s) - set(b"ACGT") for s in seqs)
    scoring = sa.Scoring.from_names(method, "dnafull", **gaps)
    store = sa.SequenceStore.from_sequences(seqs)
    pairs = packed_pairs(12)
    assert len(pairs) == 66 == store.pairs
    score, ident, cols, _ = triangle_reference(scoring, seqs, pairs)
    assert np.array_equal(score, oracle.align(store, scoring, triangular=True))
    alike = 0
    for i, j in pairs[::7]:   # (the walk again, for its columns: every seventh pair)
        alike += kinds_of_columns(scoring, seqs[i], seqs[j], traceback_ref.align_pair(scoring, seqs[i], seqs[j], i, j))[1]
    print(f"{method} dnafull {gaps}: {alike} columns of {len(pairs[::7])} alignments score as a match without being equal")
    assert alike >= 5, "no column tells equal codes from codes that score as a match"
    with sa.Context(store, scoring, 0) as ctx:
        got = device_identity(ctx, 0, len(pairs), COLUMNS)
        again = device_identity(ctx, 0, len(pairs), COLUMNS)
    check_all(f"{method} dnafull {gaps}", got, score, ident, cols, lens, pairs, COLUMNS)
    assert all(again[name].tobytes() == got[name].tobytes() for name in OUTPUTS)
