"""GPU (-m gpu): the tie rule of the alignments for chosen pairs (include/seqalign_hip.h, csrc/sa_traceback.hip), exactly, on
column sequences of 3 to 6 strips of 64 columns.

tests/test_gpu_traceback.py pins records and CIGARs byte for byte on sequences of at most 80 residues: two strips, one strip
crossing in the walk.  What decides a tie beyond column 128 is device code of its own -- the sweep restated from
sa_k_pair_per_wave, the fill's address arithmetic against sa_tb_cell_offset in the walk, the records at lane 0 of strips
2, 3, ... that come out of the boundary column, the kilobyte window crossing several strips, the SW end cell reduced over
lanes that each saw several strips -- and a wrong choice among equally good moves there is still a valid alignment of the
right score.  Here every record and every CIGAR is compared, field by field, with tests/traceback_ref.py (plain Python over
full tables, no code shared with the library).

Inputs.  Four-letter DNA without IUPAC codes (four letters make ties everywhere): row lengths 61, 62, 63, 64, 97, 130, 150,
200 (every residue of m mod 4: a strip has m + 63 lines rounded up to a multiple of four), column lengths at the strip edges
129, 191, 192, 193, 255, 256, 257, 320, three columns per row; 320 x 65 and 257 x 129 (a long row against a short
multi-strip column); two planted Smith-Waterman pairs (below); every pair in both orders (the mirror): 56 pairs.  Under
BLOSUM62 the same store read as proteins (A, C, G, T are residues of that table too) and behind it the repeats (AW)^100,
(WA)^110, A^129, A^193 and (AW)^50 A (AW)^60, every ordered pair of them: 76 pairs.

Sensitivity, from the reference alone (asserted on the CPU before the device is asked): traceback_ref.align_pair(...,
flipped_ties=True) walks the same tables with the other order among equally good moves (NW: up before diagonal; Gotoh / SW:
X / Y before diagonal), and per scoring at least half of the pairs must come out with another CIGAR -- a device that
breaks ties differently cannot pass.  Counts of these inputs (pairs whose CIGAR differs / pairs):

    nw dnafull gap 2 ............ 46 / 56        nw blosum62 gap 0 ........... 44 / 76
    ga dnafull 3 / 1 ............ 54 / 56        ga blosum62 3 / 1 ........... 74 / 76
    sw nuc44 3 / 1 .............. 52 / 56        sw blosum62 3 / 1 ........... 56 / 76
    ga dnafull 0 / 0 ............ 54 / 56
    sw dnafull 4 / 4 ............ 52 / 56
    ga dnafull 3 / 7 ............ 56 / 56

(NW under BLOSUM62 has zero gaps because with gaps of 1 .. 4 its eight distinct entries over A, C, G, T leave too few ties
between up and diagonal: 32, 34, 28 and 26 of the 76 pairs, under the half; NW with a cheap gap is pinned on the +5 / -4
table.  The repeats themselves tie mostly between diagonal and left, which the flipped walk does not exchange: they add
the plateaus -- A^129 against A^193 has 65 equal maxima in row 129, strips 2 and 3 -- not the count.)

The SW end cell: in `crossed` the row sequence carries the motifs P .. Q and the column sequence Q .. P between fillers that
match nothing (G against T), so M attains its maximum at (end of P, end of P) -- small row, column 170, strip 2 -- and at
(end of Q, end of Q) -- large row, column 40, strip 0: the cell the contract picks (smallest row) is not in the lowest
strip that holds a maximum, and a reduction that prefers what a lane saw first, or the lower column, picks the other.  In
`doubled` one motif occurs twice in both (four maxima, strips 0 and 2).  Both properties are asserted on the reference's M."""
import numpy as np
import pytest

from tests import traceback_ref
from tests.synth import make_dna_set
from tests.test_gpu_traceback import FIELDS

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (61, 62, 63, 64, 97, 130, 150, 200)
COLUMN_LENGTHS = (129, 191, 192, 193, 255, 256, 257, 320)

DNA_SCORINGS = [
    ("nw", "dnafull", dict(gap_pen=2)), ("ga", "dnafull", dict(gap_open=3, gap_extend=1)), ("sw", "nuc44", dict(gap_open=3, gap_extend=1)),
    ("ga", "dnafull", dict(gap_open=0, gap_extend=0, equal_affine_to_nw=False)),   # zero gaps
    ("sw", "dnafull", dict(gap_open=4, gap_extend=4)),                               # open == extend under SW
    ("ga", "dnafull", dict(gap_open=3, gap_extend=7)),                               # |open| < |extend|: the pair-per-wave score kernels too
]
PROTEIN_SCORINGS = [("nw", "blosum62", dict(gap_pen=0)), ("ga", "blosum62", dict(gap_open=3, gap_extend=1)), ("sw", "blosum62", dict(gap_open=3, gap_extend=1))]


def scoring_id(v):
    return v if isinstance(v, str) else "-".join(str(x) for x in v.values() if x is not False)


def dna(length: int, seed: int) -> bytes:
    return make_dna_set(1, length, length, seed)[0]


def two_letters(length: int, seed: int, letters: bytes) -> bytes:
    return bytes(letters[ch in b"GT"] for ch in dna(length, seed))


def dna_case():
    """sequences and the unordered pairs (lo, hi), lo the row sequence; planted = {name: (lo, hi)}"""
    seqs = [dna(m, 100 + m) for m in ROW_LENGTHS] + [dna(n, 500 + n) for n in COLUMN_LENGTHS]
    pairs = [(i, 8 + (i + d) % 8) for i in range(8) for d in (0, 3, 5)]   # every row length against three column lengths
    # a long row sequence against a short multi-strip column: the 65 and the 129 sit behind every row of 320 and 257
    seqs += [dna(65, 31), dna(129, 32)]
    pairs += [(8 + COLUMN_LENGTHS.index(320), 16), (8 + COLUMN_LENGTHS.index(257), 17)]
    # the planted motifs: 30 residues over A and C, equal under the table whatever the letters; fillers G (rows) and T (columns)
    p, q = two_letters(30, 41, b"AC"), two_letters(30, 42, b"AC")
    assert p != q
    seqs += [b"G" * 20 + p + b"G" * 90 + q + b"G" * 20, b"T" * 10 + q + b"T" * 100 + p + b"T" * 30]     # crossed: 190 x 200
    seqs += [b"G" * 20 + p + b"G" * 90 + p + b"G" * 20, b"T" * 10 + p + b"T" * 100 + p + b"T" * 30]     # doubled
    planted = {"crossed": (18, 19), "doubled": (20, 21)}
    pairs += list(planted.values())
    assert all(not set(s) - set(b"ACGT") for s in seqs)
    return seqs, pairs, planted


PROTEIN_REPEATS = [b"AW" * 100, b"WA" * 110, b"A" * 129, b"A" * 193, b"AW" * 50 + b"A" + b"AW" * 60]


def protein_case():
    """the DNA store read as proteins (A, C, G, T are residues of BLOSUM62 too) and, behind it, the repeats: every pair of them"""
    seqs, pairs, _ = dna_case()
    first = len(seqs)
    seqs = seqs + PROTEIN_REPEATS
    pairs = pairs + [(a, b) for a in range(first, len(seqs)) for b in range(a + 1, len(seqs))]
    return seqs, pairs, {}


def reference(scoring, seqs, pairs):
    """per unordered pair, one fill of the full tables: the contract's alignment and the other tie order's, in both index orders"""
    want, other, M = {}, {}, {}
    for lo, hi in pairs:
        tabs = traceback_ref.tables(scoring, *traceback_ref.canonical(scoring, seqs[lo], seqs[hi], lo, hi))
        M[lo, hi] = tabs[0]
        for a, b in ((lo, hi), (hi, lo)):
            want[a, b] = traceback_ref.align_pair(scoring, seqs[a], seqs[b], a, b, tabs=tabs)
            other[a, b] = traceback_ref.align_pair(scoring, seqs[a], seqs[b], a, b, flipped_ties=True, tabs=tabs)
            assert other[a, b]["score"] == want[a, b]["score"]
    return want, other, M


def maxima(M):
    best = max(max(row[1:]) for row in M[1:])
    return best, [(r, c) for r in range(1, len(M)) for c in range(1, len(M[0])) if M[r][c] == best]


def strip_of(cell):
    return (cell[1] - 1) >> 6


CASES = [pytest.param("dna", *s, id="dna-" + "-".join(map(scoring_id, s))) for s in DNA_SCORINGS] + \
        [pytest.param("protein", *s, id="protein-" + "-".join(map(scoring_id, s))) for s in PROTEIN_SCORINGS]


@pytest.mark.parametrize("kind,method,matrix,gaps", CASES)
def test_ties_beyond_the_second_strip_equal_the_python_restatement(kind, method, matrix, gaps, sa):
    seqs, unordered, planted = dna_case() if kind == "dna" else protein_case()
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    assert scoring.method == {"nw": 0, "ga": 1, "sw": 2}[method]
    lens = [len(s) for s in seqs]
    if kind == "dna":
        have = {(lens[lo], lens[hi]) for lo, hi in unordered}
        assert {m for m, _ in have} >= set(ROW_LENGTHS) and {n for _, n in have} >= set(COLUMN_LENGTHS) and {(320, 65), (257, 129)} <= have
        assert {m % 4 for m in ROW_LENGTHS} == {0, 1, 2, 3}
    assert all(lo < hi and 3 <= (lens[hi] + 63) // 64 <= 6 or (lens[lo], lens[hi]) == (320, 65) for lo, hi in unordered)   # 3 to 6 strips

    # ---- on the CPU, from the reference alone ----
    want, other, M = reference(scoring, seqs, unordered)
    pairs = np.array(sorted(want), np.int32)
    assert len(pairs) == 2 * len(unordered) >= 40
    sensitive = sum(want[a, b]["cigar"] != other[a, b]["cigar"] for a, b in want)
    print(f"{kind} {method} {matrix} {gaps}: the other tie order changes the CIGAR of {sensitive} of {len(want)} pairs")
    assert 2 * sensitive >= len(want), f"only {sensitive} of {len(want)} pairs depend on the tie order"
    if method == "sw" and planted:
        best, cells = maxima(M[planted["crossed"]])
        strips = {strip_of(cell) for cell in cells}
        assert best > 0 and len(strips) >= 2 and strip_of(min(cells)) > min(strips), (best, cells)   # (min: smallest r, then smallest c)
        end = want[planted["crossed"]]
        assert (end["a_end"], end["b_end"]) == min(cells)
        best, cells = maxima(M[planted["doubled"]])
        assert len(cells) >= 4 and len({strip_of(cell) for cell in cells}) >= 2 and len({r for r, _ in cells}) >= 2, (best, cells)

    # ---- the device ----
    store = sa.SequenceStore.from_sequences(seqs)
    got = sa.hip_alignments(store, scoring, pairs)
    assert len(got.records) == len(pairs)
    assert np.array_equal(got.records["cigar_off"], np.cumsum(got.records["cigar_len"].astype(np.int64)) - got.records["cigar_len"])
    assert int(got.records["cigar_len"].sum()) == len(got.cigar)
    for t, (a, b) in enumerate(pairs.tolist()):
        have = {f: int(got.records[t][f]) for f in FIELDS}
        have["cigar"] = got.runs(t)
        m, n = sorted((a, b))
        assert have == want[a, b], (f"{method} {matrix} {gaps} pair {t} = ({a}, {b}), rows {lens[m]} x columns {lens[n]} ({(lens[n] + 63) // 64} strips):\n"
                                    f" got  {have}\n want {want[a, b]}\n other tie order {other[a, b]['cigar']}")
    if gaps.get("gap_extend", 0) > gaps.get("gap_open", 0):
        # |open| < |extend| is also what the planner sends to sa_k_pair_per_wave: the alignments' scores are its entries
        matrix_entries = sa.hip_align(store, scoring, triangular=True)
        lo, hi = pairs.min(axis=1).astype(np.int64), pairs.max(axis=1).astype(np.int64)
        assert np.array_equal(got.records["score"], matrix_entries[hi * (hi - 1) // 2 + lo])
