"""Stores that put every class of one packed bundle on the lean way of pk_tile (sa_systolic_pk.inc), shared by
tests/test_gpu_token_classes.py (the device runs) and tests/test_plan_host.py (which arranged level every tile streams,
from the planner, without a device).

A store is ROWS rows of ROW_MIN..ROW_MAX residues over all 23 letters the scoring accepts, and behind them three columns
per class K of the bundle, of G K - (G - 1), G K - 3 and G K residues: one column pair and one column paired with itself, at
both ends of the class.  With SA_HIP_CHUNK = CHUNK a full tile is wpb x 64/G x 2 rows (32 to 128): the first 256 rows of
every column are tiles of the 256-row arranged block, the tiles from row 256 to the last whole tile are each their own
block, and the rows behind the last whole tile are a partial tile that derives its tokens."""
from tests.synth import _make

ALPHA23 = b"ARNDCQEGHILKMFPSTWYVBZX"  # (the alphabet of tools/gpu_fuzz.py: B, Z, X are the highest residue codes)
ROWS, ROW_MIN, ROW_MAX, CHUNK = 400, 16, 60, 2
KMAX = {8: 24, 16: 64}
BUNDLES = [(8, 1), (8, 9), (8, 17)] + [(16, klo) for klo in range(13, 62, 8)]  # (lanes per group, KLO): sa_pk_bundle_klo
LOW_K_TWO_WAY = [(16, 13), (16, 21)]  # the stores that get a one-residue row: the two-way u16 form at K = 13 ...
METHODS = [("nw", dict(gap_pen=4)), ("ga", dict(gap_open=10, gap_extend=1)), ("sw", dict(gap_open=10, gap_extend=1))]
MATRIX = "blosum62"


def bundle_classes(g, klo):
    return list(range(klo, min(klo + 8, KMAX[g] + 1)))


def column_lengths(g, k):
    return [g * k - (g - 1), g * k - 3, g * k]


def first_column(g, klo, k, short_row=False):
    """index of the first of the three columns of class k"""
    return ROWS + int(short_row) + 3 * (k - klo)


def store_sequences(g, klo, short_row=False):
    """short_row: a one-residue row in front (the shortest sequence of a store decides how many frame shifts the bound
    allows for, hence the form of the 16-lane classes)"""
    seed = 100 * g + klo
    rows = _make(ROWS, ROW_MIN, ROW_MAX, seed, ALPHA23)
    lens = [n for k in bundle_classes(g, klo) for n in column_lengths(g, k)]
    cols = [s[:n] for s, n in zip(_make(len(lens), max(lens), max(lens), seed + 1, ALPHA23), lens)]
    return ([ALPHA23[klo % 23:klo % 23 + 1]] if short_row else []) + rows + cols


def store_lengths(g, klo, short_row=False):
    return [len(s) for s in store_sequences(g, klo, short_row)]
