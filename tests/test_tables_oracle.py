"""CPU: the yardstick of tests/test_gpu_tables.py is pinned first.  For substitution tables that are NOT one of the named
matrices (tests/tables.py: an asymmetric one, and one with the extremes -127 / +127 on top of it) the oracle must equal

  1. the reference's own functions, whose SEQ_LUT / SUB_MAT data RefLib.set_tables overwrites at run time -- live through
     oracle/_ref/libseqalign_ref.so where the reference was present at build time, else the answers that library gave to the
     very same calls, stored by tools/make_golden.py (tests/golden/tables_vs_ref.npz);
  2. the plain-Python restatement tests/traceback_ref.tables(), literal and independent, on 30 short pairs;

and 3. the tables must be worth testing with: the oracle on sub.T differs from the oracle on sub for at least half of the
pairs.  The index order is the point: NW reads sub[code of i][code of j], Gotoh / SW sub[code of j][code of i] (i < j, j the
column sequence; reference src/bio/method/nw.c:23,29, ga.c:46, sw.c:39) -- with symmetric tables nothing can tell the
two apart, and every named matrix is symmetric (test_every_named_matrix_is_symmetric)."""
import json

import numpy as np
import pytest

from tests import extremal as ex
from tests import tables as tb
from tests import traceback_ref
from tests.oracle_binding import ROOT, RefLib, ref_available

GOLDEN = ROOT / "tests" / "golden" / "tables_vs_ref.npz"

GAPS, METHODS = tb.GAPS, tb.METHODS


def table(name: str) -> np.ndarray:
    base = tb.asymmetric(1, -4, 11)
    return {"asymmetric": base, "extremes": tb.with_extremes(base, -127, 127)}[name]


TABLES = ["asymmetric", "extremes"]


def random_store(sa):
    """40 sequences of 1..160 residues over all 24 codes"""
    lens = np.random.default_rng(41).integers(1, 161, 40)
    lens[:2] = (1, 160)
    return sa.SequenceStore.from_sequences(tb.random_sequences(lens, 42))


def live_reference(method, gaps, lut, sub, store) -> dict:
    ref = RefLib(method, "blosum62", **gaps)
    try:
        ref.set_tables(lut, sub)
        p = ref.params()
        assert np.array_equal(p["lut"], lut) and np.array_equal(p["sub"], sub)  # the reference's code reads what was written
        return dict(lut=p["lut"], sub=p["sub"], blob=store.blob.copy(), meta=store.meta.copy(), tri=ref.align(store, triangular=True))
    finally:
        ref.close()


def stored_calls(sa):
    """every call whose answer GOLDEN keeps: (key, method, gaps, lut, sub, store)"""
    store = random_store(sa)
    for name in TABLES:
        for method in METHODS:
            yield f"{method}_{name}", method, GAPS[method], tb.lut24(), table(name), store


def reference(key, method, gaps, lut, sub, store) -> dict:
    stored = None
    if GOLDEN.exists():
        with np.load(GOLDEN) as z:
            stored = {name[len(key) + 1:]: z[name] for name in z.files if name.startswith(key + "/")}
    if ref_available():
        live = live_reference(method, gaps, lut, sub, store)
        if stored:  # the fixture is what the reference says today
            assert np.array_equal(stored["tri"], live["tri"]), f"{GOLDEN.name} {key}: regenerate it with tools/make_golden.py"
        return live
    assert stored, f"{GOLDEN.name} holds no entry {key}: regenerate it with tools/make_golden.py"
    assert json.loads(str(stored.pop("gaps"))) == gaps
    # (the stored answers belong to exactly this input)
    assert np.array_equal(stored["blob"], store.blob) and np.array_equal(stored["meta"], store.meta)
    assert np.array_equal(stored["lut"], lut) and np.array_equal(stored["sub"], sub)
    return stored


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("method", METHODS)
def test_oracle_equals_the_reference_on_a_table_given_as_data(method, name, oracle, sa):
    store = random_store(sa)
    assert store.num == 40 and store.max == 160 and int(store.meta[:, 1].min()) == 1
    sub, lut = table(name), tb.lut24()
    scoring = tb.scoring_with(sa, method, GAPS[method], sub, lut)
    assert scoring.matrix_name == "" and scoring.method_name == method
    p = reference(f"{method}_{name}", method, GAPS[method], lut, sub, store)
    want = oracle.align(store, scoring, triangular=True)
    assert np.array_equal(p["tri"], want), f"{(p['tri'] != want).sum()} of {want.size} pairs differ from the reference"
    # 3. the sensitivity guard: a table on which the wrong index order would go unnoticed is too tame to test with
    swapped = oracle.align(store, tb.transposed(scoring), triangular=True)
    differ = int((swapped != want).sum())
    print(f"{method} {name}: the oracle on sub.T differs on {differ} of {want.size} pairs")
    assert 2 * differ >= want.size, f"{method} {name}: sub.T changes only {differ} of {want.size} scores"


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("method", METHODS)
def test_oracle_equals_the_python_restatement(method, name, oracle, sa):
    scoring = tb.scoring_with(sa, method, GAPS[method], table(name))
    lens = np.random.default_rng(7).integers(1, 26, 60)
    seqs = tb.random_sequences(lens, 8)
    for t in range(30):
        lo, hi = seqs[2 * t], seqs[2 * t + 1]  # lo: the earlier (row) sequence, hi: the later (column) one
        M, _, _ = traceback_ref.tables(scoring, [int(scoring.lut[c]) for c in lo], [int(scoring.lut[c]) for c in hi])
        want = max(max(row) for row in M) if method == "sw" else M[len(lo)][len(hi)]
        got = oracle.pair(scoring, hi, lo)
        assert got == want, f"{method} {name} pair {t} ({len(lo)} x {len(hi)}): oracle {got}, restatement {want}"


def test_every_named_matrix_is_symmetric(sa):
    """the recorded reason an index order could be wrong unseen: no named matrix can tell sub[a][b] from sub[b][a].  It is
    also why staging a transposed table for Gotoh / SW changes no byte of what any named matrix stages."""
    for name in sa.matrix_names():
        sub = sa.Scoring.from_names("nw", name, gap_pen=1).sub.reshape(24, 24)
        assert np.array_equal(sub, sub.T), name
        assert -128 < sub.min() and sub.max() < 128, name


# ---- the builders themselves ----------------------------------------------------------------------------------------------
def test_asymmetric_tables():
    for seed, lo, hi in ((1, -4, 11), (2, -9, 11), (3, -100, 100)):
        sub = tb.asymmetric(seed, lo, hi)
        assert sub.shape == (576,) and sub.dtype == np.int32 and lo <= sub.min() and sub.max() <= hi
        m = sub.reshape(24, 24)
        assert not np.array_equal(m, m.T)
        tb.check_shape(sub)
        assert np.array_equal(sub, tb.asymmetric(seed, lo, hi))  # a function of the seed


@pytest.mark.parametrize("method", METHODS)
def test_with_extremes_and_what_the_input_builders_make_of_it(method, sa):
    base = tb.asymmetric(1, -4, 11)
    sub = tb.with_extremes(base, -127, 127)
    m = sub.reshape(24, 24)
    x, b, c = tb.extreme_places(base)
    assert m[x, x] == 127 == m.max() and m[b, c] == -127 == m.min() and b != c and m[c, b] != -127
    assert (sub != base).sum() == 2
    tb.check_shape(sub)
    # tests/extremal.py finds the extremes, and its bottom pair fills the cells with the minimum under the method's own order
    scoring = tb.scoring_with(sa, method, GAPS[method], sub)
    view = tb.builder_view(scoring)
    assert ex.best_residue(view) == tb.LETTERS24[x].encode()
    row, col = ex.worst_pair(view)
    assert traceback_ref._sim(scoring, int(scoring.lut[row[0]]), int(scoring.lut[col[0]])) == -127
    assert traceback_ref._sim(scoring, int(scoring.lut[col[0]]), int(scoring.lut[row[0]])) != -127


def test_luts_and_stores():
    lut = tb.lut24()
    assert sorted(lut[lut >= 0]) == list(range(24)) and (lut >= 0).sum() == 24
    many = tb.lut_many()
    assert many[ord("J")] == many[ord("L")] and many[ord("a")] == many[ord("A")] and many[ord("w")] == many[ord("W")]
    assert many[ord(tb.REFUSED[0])] == 24 and many[ord(tb.REFUSED[1])] == -1
    assert len(tb.MANY_LETTERS) == 24 + 4 + 26  # (23 letters and '*'; J, U, O and '.'; then all of a..z)
    codes = {int(many[ch]) for ch in tb.MANY_LETTERS}
    assert codes == set(range(24))

    class S:  # (what every_code_in_rows_and_columns reads of a Scoring)
        pass
    s = S()
    s.lut = lut
    for shortest in (1, 16):
        seqs = tb.order_store(shortest)
        lens = [len(q) for q in seqs]
        assert min(lens) == shortest and sorted(lens[41 - shortest:]) == sorted([n for n in tb.COLUMN_LENGTHS if n >= shortest] * 2)
        assert tb.every_code_in_rows_and_columns(s, seqs)
    assert 16000 < sum(map(len, tb.order_store())) < 18000


# ---- the case lists of tests/test_gpu_tables.py, checked against the planner without a device ---------------------------
from tests.planner_limits import PACKED_FORMS, columns_by_form, planner, unreached_forms  # noqa: E402,F401  (planner: a fixture)


def test_order_stores_reach_every_packed_form(sa, planner):
    """the stores of test_index_order_on_every_family: with the columns added for forms that end between two of the fixed
    lengths no admitted form is left without a column, and the two stores together admit all three packed forms"""
    for method in METHODS:
        scoring = tb.scoring_with(sa, method, GAPS[method], tb.asym())
        reached = set()
        for shortest in (1, 16):
            lim = planner(scoring, max(tb.COLUMN_LENGTHS), shortest)
            extra = [lanes * k for _, lanes, k in unreached_forms([len(s) for s in tb.order_store(shortest)], lim)]
            lens = [len(s) for s in tb.order_store(shortest, extra=extra)]
            assert (max(lens), min(lens)) == (max(tb.COLUMN_LENGTHS), shortest) and not unreached_forms(lens, lim)
            reached |= set(columns_by_form(lens, lim))
        assert reached == set(PACKED_FORMS) | {"s32"}, (method, reached)


def test_edge_entries_lie_on_both_sides_of_their_condition(sa, planner):
    """the entries of test_table_entries_at_the_admission_edges: for every method and condition the planner admits the first
    to a family above the second's, whatever the shortest sequence of the store (7: top and bottom stores, 1: the frames
    store)"""
    for method in METHODS:
        for condition in tb.CONDITIONS:
            gaps, values, which = tb.edge_case(method, condition)
            ranks = []
            for value in values:
                scoring = tb.scoring_with(sa, method, gaps, tb.edge_table(value, which))
                assert scoring.method_name == method
                m = np.asarray(scoring.sub).reshape(24, 24)
                assert (m.max() if which == "max" else m.min()) == value
                both = {tb.family_rank(planner(scoring, max(tb.EDGE_LENGTHS), shortest)) for shortest in (7, 1)}
                assert len(both) == 1, (method, condition, value)
                ranks.append(both.pop())
            assert ranks[0] > ranks[1], (method, condition, values, ranks)
