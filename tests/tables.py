"""Substitution tables and luts as DATA: what `sa_scoring.sub` / `sa_scoring.lut` may hold besides the named matrices --
tables that are not symmetric, tables with a chosen minimum and maximum (the admission edges of
sequencealigner_amd/csrc/sa_limits.cpp), luts over all 24 codes, with several letters per code and lower-case letters.
Numpy only; used by tests/test_tables_oracle.py (CPU) and tests/test_gpu_tables.py.

The index order the tables are read in (reference src/bio/method/nw.c:23,29; ga.c:46; sw.c:39), i < j, j the column sequence:
NW sub[code of i][code of j], Gotoh / SW sub[code of j][code of i]."""
from __future__ import annotations

import dataclasses

import numpy as np

from sequencealigner_amd.binding import METHOD_NW
from tests import extremal as ex

SUB_DIM = 24
LUT_SIZE = 128
LETTERS24 = "ARNDCQEGHILKMFPSTWYVBZX*"  # the order of the protein matrices: codes 20..23 are B Z X *
REFUSED = (b"@", b"?")  # LUT_MANY maps the first to 24 and the second to -1: both "Invalid character"


def asymmetric(seed: int, lo: int, hi: int) -> np.ndarray:
    """576 entries in [lo, hi], sub != sub.T: the off-diagonal ones uniform in [lo, hi - 1], every diagonal entry uniform
    between the largest entry of its row and column + 1 and hi -- the strict maximum of both, so that a homopolymer of the
    residue with the largest diagonal entry is still the best a sequence can do (tests/extremal.py)"""
    assert hi - lo >= 4
    rng = np.random.default_rng(seed)
    sub = rng.integers(lo, hi, (SUB_DIM, SUB_DIM))  # (hi exclusive)
    off = ~np.eye(SUB_DIM, dtype=bool)
    for x in range(SUB_DIM):
        top = max(sub[x, off[x]].max(), sub[off[:, x], x].max())
        sub[x, x] = rng.integers(top + 1, hi + 1)
    check_shape(sub)
    assert (sub != sub.T).sum() > SUB_DIM * SUB_DIM // 2, "hardly asymmetric: choose a wider range"
    return sub.astype(np.int32).reshape(-1)


def check_shape(sub) -> None:
    """the diagonal is the strict maximum of every row and column"""
    sub = np.asarray(sub).reshape(SUB_DIM, SUB_DIM)
    off = ~np.eye(SUB_DIM, dtype=bool)
    for x in range(SUB_DIM):
        assert sub[x, x] > sub[x, off[x]].max() and sub[x, x] > sub[off[:, x], x].max(), x


def extreme_places(base) -> tuple[int, int, int]:
    """(x, b, c): with_extremes puts the maximum at [x][x] -- where the largest diagonal entry of `base` is, the first among
    equals -- and the minimum at [b][c], the first smallest off-diagonal entry of `base`; all three among the codes 0..22,
    whose letters are upper-case ones (tests/extremal.py builds its sequences from A..Z, code 23 is '*')"""
    sub = np.asarray(base).reshape(SUB_DIM, SUB_DIM)[:SUB_DIM - 1, :SUB_DIM - 1]
    n = SUB_DIM - 1
    x = int(np.argmax(np.diag(sub)))
    masked = np.where(np.eye(n, dtype=bool), np.iinfo(np.int64).max, sub.astype(np.int64))
    b, c = divmod(int(np.argmin(masked)), n)
    return x, b, c


def with_extremes(base, smin: int, smax: int) -> np.ndarray:
    """a copy of `base` whose only minimum smin is the off-diagonal entry [b][c] and whose only maximum smax is the diagonal
    entry [x][x] (extreme_places); [c][b] keeps its value > smin: the two index orders reach different bottoms"""
    sub = np.asarray(base).reshape(SUB_DIM, SUB_DIM).astype(np.int64)
    assert smin < sub.min() and sub.max() < smax, (smin, int(sub.min()), int(sub.max()), smax)
    x, b, c = extreme_places(sub)
    sub[x, x] = smax
    sub[b, c] = smin
    assert sub[c, b] != smin and b != c
    assert (sub == smin).sum() == 1 and (sub == smax).sum() == 1 and sub.min() == smin and sub.max() == smax
    return sub.astype(np.int32).reshape(-1)


def lut24(letters: str = LETTERS24) -> np.ndarray:
    """letter k of `letters` -> code k, every other byte -1: a lut over all 24 codes"""
    assert len(letters) == SUB_DIM and len(set(letters)) == SUB_DIM
    lut = np.full(LUT_SIZE, -1, np.int32)
    for code, ch in enumerate(letters):
        lut[ord(ch)] = code
    return lut


def lut_many() -> np.ndarray:
    """lut24 plus: several letters on one code (J with L, U with C, O with K, '.' with '*'), every lower-case letter on the
    code of its upper-case one, and the two refused letters: '@' -> 24 (one past the table), '?' -> -1"""
    lut = lut24()
    for extra, known in (("J", "L"), ("U", "C"), ("O", "K"), (".", "*")):
        lut[ord(extra)] = lut[ord(known)]
    for ch in range(ord("A"), ord("Z") + 1):
        lut[ch + 32] = lut[ch]
    lut[ord("@")] = SUB_DIM
    lut[ord("?")] = -1
    return lut


MANY_LETTERS = sorted(ch for ch in range(LUT_SIZE) if 0 <= lut_many()[ch] < SUB_DIM)


def scoring_with(sa, method: str, gaps: dict, sub, lut=None):
    """a Scoring with the table (and lut) given as data: no matrix name"""
    base = sa.Scoring.from_names(method, "blosum62", **gaps)
    return dataclasses.replace(base, sub=np.ascontiguousarray(sub, np.int32).reshape(-1),
                               lut=lut24() if lut is None else np.ascontiguousarray(lut, np.int32), matrix_name="")


def builder_view(scoring):
    """the scoring tests/extremal.py is to derive its letters from: that module reads sub[row residue][column residue], which
    is the order of NW; for Gotoh / SW the cell of row residue r and column residue c holds sub[c][r], so the builders get
    the transposed table.  The pair worst_pair returns then fills the cells of the bottom stores with the table's minimum
    under the method's own order."""
    return scoring if scoring.method == METHOD_NW else transposed(scoring)


def transposed(scoring):
    return dataclasses.replace(scoring, sub=np.ascontiguousarray(scoring.sub.reshape(SUB_DIM, SUB_DIM).T).reshape(-1))


def raw_store(sa, seqs):
    """a SequenceStore of the bytes as they are (SequenceStore.from_sequences upper-cases: lower-case letters would never
    reach the lut)"""
    items = [bytes(s) for s in seqs]
    lens = np.array([len(s) for s in items], np.int64)
    offs = np.zeros(len(items), np.int64)
    offs[1:] = np.cumsum(lens[:-1] + 1)
    blob = np.frombuffer(b"\0".join(items) + b"\0", dtype=np.uint8).copy()
    return sa.SequenceStore(blob=blob, meta=np.ascontiguousarray(np.stack([offs, lens], axis=1).astype(np.int32)), num=len(items), max=int(lens.max()))


def random_sequences(lengths, seed: int, letters=LETTERS24) -> list[bytes]:
    """one sequence per length, uniform over `letters` (a str or a list of byte values): all 24 codes occur"""
    pool = np.frombuffer(letters.encode(), np.uint8) if isinstance(letters, str) else np.array(letters, np.uint8)
    rng = np.random.default_rng(seed)
    return [pool[rng.integers(0, pool.size, int(n))].tobytes() for n in lengths]


def every_code_in_rows_and_columns(scoring, seqs) -> bool:
    """every code 0..23 occurs in a row (the first half of the store: rows of the columns behind it) and in a column (the
    second half)"""
    def codes(part):
        return {int(scoring.lut[ch]) for s in part for ch in s}
    half = len(seqs) // 2
    return codes(seqs[:half]) >= set(range(SUB_DIM)) and codes(seqs[half:]) >= set(range(SUB_DIM))


# ---- the stores of tests/test_gpu_tables.py (their shapes are verified on the CPU by tests/test_tables_oracle.py) ----
ROW_LENGTHS = list(range(1, 41))
# the smallest lengths that still touch: the 64-column strips of the pair-per-wave kernels (63..65, 127..129), the last 8-lane
# class and the first class behind it (192, 193), the first 16-lane classes (208, 209), the f16 cut-off (832, 833), the last
# packed width (1023..1025) and two and three strips of the strip-mined s32 kernels (1025, 2049)
COLUMN_LENGTHS = [8, 9, 63, 64, 65, 127, 128, 129, 192, 193, 208, 209, 832, 833, 1023, 1024, 1025, 2049]


def order_store(shortest: int = 1, seed: int = 5, extra=()) -> list[bytes]:
    """rows of `shortest`..40 residues, then every column length (no shorter than `shortest`) twice in a shuffled order (fixed
    seed), over all 24 codes; then the columns of `extra`, each twice"""
    cols = np.array([n for n in COLUMN_LENGTHS if n >= shortest] * 2)
    np.random.default_rng(seed).shuffle(cols)
    return random_sequences([n for n in ROW_LENGTHS if n >= shortest] + cols.tolist() + sorted(extra) * 2, seed + 1)


# ---- the cases of tests/test_gpu_tables.py (checked against the planner on the CPU by tests/test_tables_oracle.py) ----
METHODS = ["nw", "ga", "sw"]
GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}
# gaps of 0: the profile adds nothing to a table entry.  Open 0 / extend 0 is a Gotoh scoring of the C ABI; only the default
# of Scoring.from_names turns it into NW
ZERO = {"nw": dict(gap_pen=0), "ga": dict(gap_open=0, gap_extend=0, equal_affine_to_nw=False), "sw": dict(gap_open=0, gap_extend=0)}
EDGE_LENGTHS = ex.class_lengths([8, 64, 192, 208, 1024]) + [1025]
CONDITIONS = ["smax", "smin", "pmax", "s32-floor", "pk-floor"]


def asym() -> np.ndarray:
    """the asymmetric table of the GPU cases: entries in [-4, 11]"""
    return asymmetric(1, -4, 11)


def edge_case(method: str, condition: str):
    """(gaps, (last admitted entry, first refused entry), which extreme) for one table condition of sa_limits.cpp, the entry
    derived from the gaps: pconst is what the profile adds to every entry (NW 2 |g|, Gotoh |o| + |e|, SW |o|), and Gotoh's
    first real column carries |o| - |e| on top.  smax > 127 and smin + pconst < -127 decide only where pmax > 127 and
    smin < -127 do not come first: with gaps of 0."""
    gaps = ZERO[method] if condition in ("smax", "s32-floor") else GAPS[method]
    g, o, e = gaps.get("gap_pen", 0), gaps.get("gap_open", 0), gaps.get("gap_extend", 0)
    pconst, top = {"nw": (2 * g, 2 * g), "ga": (o + e, 2 * o), "sw": (o, o)}[method]
    if condition == "smax":  # smax > 127
        return gaps, (127, 128), "max"
    if condition == "smin":  # smin < -127
        return gaps, (-127, -128), "min"
    if condition == "pmax":  # pmax > 127
        return gaps, (127 - top, 128 - top), "max"
    if condition == "s32-floor":  # smin + pconst < -127
        return gaps, (-127 - pconst, -128 - pconst), "min"
    assert condition == "pk-floor"  # smin + pconst < 0
    return gaps, (-pconst, -pconst - 1), "min"


def edge_table(value: int, which: str) -> np.ndarray:
    """the asymmetric table with the entry under test as its minimum or maximum; the other extreme lies just outside it"""
    return with_extremes(asym(), value, 12) if which == "min" else with_extremes(asym(), -5, value)


def family_rank(lim: dict) -> int:
    """2: packed classes are admitted, 1: the s32 family only, 0: the pair-per-wave kernels"""
    return 2 if lim["pk"] else 1 if lim["sys_ok"] else 0
