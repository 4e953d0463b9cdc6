"""GPU (-m gpu): substitution tables and luts handed to the library as DATA (tests/tables.py) -- tables that are not
symmetric, table entries at the admission edges of sequencealigner_amd/csrc/sa_limits.cpp, the codes 20..23, luts with several
letters per code and lower-case letters -- on every kernel family against the oracle, which tests/test_tables_oracle.py pins
to the reference for exactly such tables.

`sub` is read in a fixed order (include/seqalign_hip.h): NW sub[code of i][code of j], Gotoh / SW sub[code of j][code of i],
i < j, j the column sequence.  Every named matrix is symmetric, so only a table that is not can tell whether a kernel
family keeps that order; the s8 profiles of the packed and s32 systolic kernels are built from a staged copy (sub8), the
pair-per-wave kernels and the traceback read `sub` itself.

Every comparison is np.array_equal with the oracle, and every case checks through ctx.timing_read()["kernel"] which family
ran: sa_k_systolic_pk_bundle<...> (planner_limits.BUNDLE) for the packed forms, sa_k_systolic< for the s32 family,
sa_k_pair_per_wave< for the fallback -- a silent fallback must not turn a case into a test of other code.  What a store admits
is asked of the planner (tests/planner_limits.py), never restated."""
import numpy as np
import pytest

from tests import extremal as ex
from tests import tables as tb
from tests import traceback_ref
from tests.planner_limits import BUNDLE, PACKED_FORMS, class_of, columns_by_form, forms, planner, unreached_forms  # noqa: F401  (planner: a fixture)
from tests.tables import CONDITIONS, EDGE_LENGTHS, GAPS, METHODS, asym, edge_case, edge_table, family_rank
from tests.test_gpu_traceback import FIELDS, both_orders
from tests.test_gpu_value_range import mismatch, timed_range, tri

pytestmark = pytest.mark.gpu

SWITCHES = ("SA_HIP_NO_SORT", "SA_HIP_NO_TOKENS", "SA_HIP_NO_PK", "SA_HIP_NO_PK16", "SA_HIP_FORCE_GENERIC", "SA_HIP_CHUNK")
S32, GENERIC = "sa_k_systolic<", "sa_k_pair_per_wave<"


def context(sa, monkeypatch, store, scoring, switch=None):
    """a context created under exactly one switch (or none): the switches are read when a context is created"""
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    return sa.Context(store, scoring, 0)


def column(ctx, want, j, tag):
    """column j as a packed range of its own: compared, and the kernel it ran on"""
    got, kernel = timed_range(ctx, tri(j), j)
    assert np.array_equal(got, want[tri(j):tri(j + 1)]), f"{tag}: column {j} on {kernel}: " + mismatch(got, want[tri(j):tri(j + 1)], tri(j))
    return kernel


def check_forms(ctx, lens, lim, want, tag, every_form=True):
    """the last column of every form the limits admit ran on that form (every_form: and each has one), the last column no
    form takes on the s32 family; returns the forms that ran"""
    by_form = columns_by_form(lens, lim)
    ran = set()
    for name, g, k, _ in forms(lim):
        if k == 0 or (name == "pk16-u16" and k <= lim["f16"]):  # (u16 classes: those above the f16 cut-off)
            continue
        assert by_form.get(name) or not every_form, f"{tag}: the limits {lim} admit {name}, no column of the store runs on it"
        if not by_form.get(name):
            continue
        j = by_form[name][-1]
        kernel = column(ctx, want, j, tag)
        mt = BUNDLE.match(kernel)
        assert mt and int(mt[1]) == g and (mt[3] == "true") == (name != "pk16-u16"), f"{tag}: column {j} ({lens[j]} residues, {name}) ran on {kernel}"
        assert int(mt[4]) <= class_of(lens[j], lim)[1] <= int(mt[5]), kernel
        ran.add(name)
    if by_form.get("s32"):
        kernel = column(ctx, want, by_form["s32"][-1], tag)
        assert kernel.startswith(S32 if lim["sys_ok"] else GENERIC), f"{tag}: a column no packed form takes ran on {kernel}"
        ran.add("s32" if lim["sys_ok"] else "generic")
    return ran


def whole(ctx, store, want, tag):
    got, kernel = timed_range(ctx, 0, store.pairs)
    assert np.array_equal(got, want), f"{tag}, {kernel}: " + mismatch(got, want)
    return got, kernel


# ---- 1. index order, every family -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_index_order_on_every_family(method, sa, oracle, planner, monkeypatch):
    """an asymmetric table, entries in [-4, 11], all 24 codes in rows and columns; rows of 1..40 residues, columns at the
    lengths of tables.COLUMN_LENGTHS.  One oracle matrix per store; the runs: default, store order, derived tokens, the s32
    family alone, the pair-per-wave kernels alone.  Every packed form the planner admits must have run: where the frame
    shifts of a one-residue row end a form between two of those lengths, a column as wide as the form's last admitted
    class is added (twice); where they leave a form unadmitted, a second store whose shortest sequence has 16 residues
    follows -- all three forms must have run in the end."""
    scoring = tb.scoring_with(sa, method, GAPS[method], asym())
    ran = set()
    for shortest in (1, 16):
        lim = planner(scoring, max(tb.COLUMN_LENGTHS), shortest)
        assert lim["sys_ok"] and lim["pk"], lim
        extra = [g * k for _, g, k in unreached_forms([len(s) for s in tb.order_store(shortest)], lim)]
        seqs = tb.order_store(shortest, extra=extra)
        assert tb.every_code_in_rows_and_columns(scoring, seqs)
        lens = [len(s) for s in seqs]
        assert (max(lens), min(lens)) == (max(tb.COLUMN_LENGTHS), shortest) and not unreached_forms(lens, lim)
        store = sa.SequenceStore.from_sequences(seqs)
        want = oracle.align(store, scoring, triangular=True, threads=16)
        tag = f"{method} shortest {shortest} limits {lim}"
        for switch in (None, "SA_HIP_NO_SORT", "SA_HIP_NO_TOKENS"):
            with context(sa, monkeypatch, store, scoring, switch) as ctx:
                whole(ctx, store, want, f"{tag} {switch or 'default'}")
                ran_here = check_forms(ctx, lens, lim, want, f"{tag} {switch or 'default'}")
                assert "s32" in ran_here  # (the columns of 1025 and 2049 residues: two and three strips)
                ran |= ran_here
        with context(sa, monkeypatch, store, scoring, "SA_HIP_NO_PK") as ctx:
            _, kernel = whole(ctx, store, want, f"{tag} SA_HIP_NO_PK")
            assert kernel.startswith(S32), kernel
            for n in (1024, 2049):  # the widest single-strip class, three strips
                kernel = column(ctx, want, max(j for j in range(len(lens)) if lens[j] == n), f"{tag} SA_HIP_NO_PK")
                assert kernel.startswith(S32) and kernel.endswith("strips>") == (n > 1024), kernel
        with context(sa, monkeypatch, store, scoring, "SA_HIP_FORCE_GENERIC") as ctx:
            _, kernel = whole(ctx, store, want, f"{tag} SA_HIP_FORCE_GENERIC")
            assert kernel.startswith(GENERIC), kernel
        if method == "nw" and shortest == 1:  # ... and the table is not silently symmetrised: sub.T gives other scores
            swapped = tb.transposed(scoring)
            want_t = oracle.align(store, swapped, triangular=True, threads=16)
            with context(sa, monkeypatch, store, swapped) as ctx:
                got_t, _ = whole(ctx, store, want_t, f"{tag} sub.T")
            assert 2 * int((got_t != want).sum()) >= want.size, f"{method}: sub.T changes only {(got_t != want).sum()} of {want.size} scores on the device"
        if set(PACKED_FORMS) <= ran:
            break
    assert set(PACKED_FORMS) <= ran, f"{method}: only {sorted(ran)} ran"


# ---- 2. the traceback keeps its promise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_traceback_score_is_the_packed_kernels_entry(method, sa, oracle, monkeypatch):
    """include/seqalign_hip.h: an alignment's `score` equals the score kernels' entry for that pair "even for a matrix that is
    not symmetric" -- 60 sequences of 5..120 residues, 200 pairs in both index orders, the matrix from the packed kernels"""
    scoring = tb.scoring_with(sa, method, GAPS[method], asym())
    seqs = tb.random_sequences(np.random.default_rng(3).integers(5, 121, 60), 4)
    store = sa.SequenceStore.from_sequences(seqs)
    pairs = both_orders(len(seqs), 200, 9)
    assert (pairs[:, 0] > pairs[:, 1]).sum() > 50 and (pairs[:, 0] < pairs[:, 1]).sum() > 50
    want = oracle.align(store, scoring, triangular=True)
    with context(sa, monkeypatch, store, scoring) as ctx:
        matrix, kernel = timed_range(ctx, 0, store.pairs)
        assert BUNDLE.match(kernel), kernel
        got = ctx.alignments(pairs)
    lo, hi = pairs.min(axis=1).astype(np.int64), pairs.max(axis=1).astype(np.int64)
    entry = matrix[hi * (hi - 1) // 2 + lo]
    differ = np.nonzero(got.records["score"] != entry)[0]
    assert differ.size == 0, f"{method}: {differ.size} of {len(pairs)} alignments score other than the matrix of {kernel}, first pair {pairs[differ[0]]}: " \
                             f"{got.records['score'][differ[0]]} against {entry[differ[0]]}"
    assert np.array_equal(matrix, want), f"{method}, {kernel}: " + mismatch(matrix, want)
    for t, (a, b) in enumerate(pairs):
        ref = traceback_ref.align_pair(scoring, seqs[a], seqs[b], int(a), int(b))
        have = {f: int(got.records[t][f]) for f in FIELDS}
        have["cigar"] = got.runs(t)
        assert have == ref, f"{method} pair {t} = ({a}, {b}):\n got  {have}\n want {ref}"


# ---- 3. table entries at the admission edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("condition", CONDITIONS)
@pytest.mark.parametrize("method", METHODS)
def test_table_entries_at_the_admission_edges(method, condition, sa, oracle, planner, monkeypatch):
    """with_extremes puts one entry at the last value a condition of sa_limits.cpp admits, then at the first it refuses; the
    top, bottom and frames (shortest 1) stores of tests/extremal.py fill whole columns with that entry.  What each side is
    admitted to comes from the planner; the admitted side runs there, the refused side on the next family sa_limits.cpp
    leaves it: s32 behind the packed floor, the pair-per-wave kernels behind the s32 conditions -- and behind pmax > 127 too,
    two families down from the packed kernels, because that condition ends the s32 family and the packed forms need it.
    The conditions on the largest entry alone (smax) and on the s32 floor decide only where the profile adds nothing:
    gaps of 0, Gotoh included (open 0 / extend 0 is a Gotoh scoring of the C ABI; only Scoring.from_names' default turns
    it into NW)."""
    gaps, values, which = edge_case(method, condition)
    outcomes = []
    for value in values:
        sub = edge_table(value, which)
        scoring = tb.scoring_with(sa, method, gaps, sub)
        view = tb.builder_view(scoring)
        stores = {"top": ex.top_store(view, EDGE_LENGTHS), "bottom": ex.bottom_store(view, EDGE_LENGTHS), "frames": ex.frames_store(view, 1, EDGE_LENGTHS)}
        ranks, kernels = set(), set()
        for name, seqs in stores.items():
            lens = [len(s) for s in seqs]
            store = sa.SequenceStore.from_sequences(seqs)
            lim = planner(scoring, max(lens), min(lens))
            want = oracle.align(store, scoring, triangular=True, threads=16)
            tag = f"{method} {condition} entry {value} gaps {gaps} {name} limits {lim}"
            with context(sa, monkeypatch, store, scoring) as ctx:
                _, kernel = whole(ctx, store, want, tag)
                ran = check_forms(ctx, lens, lim, want, tag, every_form=False)
            if lim["pk"]:
                assert ran & set(PACKED_FORMS), f"{tag}: {ran}"
            else:
                assert kernel.startswith(S32 if lim["sys_ok"] else GENERIC), f"{tag}: ran on {kernel}"
            ranks.add(family_rank(lim))
            kernels.add(kernel.split("<")[0])
            print(f"edge {method} {condition} entry {value} gaps {gaps} {name}: planner {lim}, ran {sorted(ran)}, dominant {kernel}")
        assert len(ranks) == 1, f"{method} {condition} {value}: the three stores are admitted to different families"
        outcomes.append(ranks.pop())
    assert scoring.method == {"nw": 0, "ga": 1, "sw": 2}[method]
    want_ranks = {"pk-floor": [2, 1], "pmax": [2, 0]}.get(condition, [1, 0])
    assert outcomes == want_ranks, f"{method} {condition}: entries {values} are admitted to {outcomes} (2 packed, 1 s32, 0 pair-per-wave), not {want_ranks}"


# ---- 4. codes and luts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_lut_with_several_letters_per_code_and_lower_case(method, sa, oracle, monkeypatch):
    scoring = tb.scoring_with(sa, method, GAPS[method], asym(), tb.lut_many())
    seqs = tb.random_sequences(list(range(1, 41)) + [64, 65, 129, 150, 150, 129], 12, tb.MANY_LETTERS)
    assert any(ch in s for s in seqs for ch in b"jou.") and tb.every_code_in_rows_and_columns(scoring, seqs)
    store = tb.raw_store(sa, seqs)
    want = oracle.align(store, scoring, triangular=True)
    same = sa.SequenceStore.from_sequences([bytes(tb.LETTERS24[int(scoring.lut[ch])].encode()[0] for ch in s) for s in seqs])
    assert np.array_equal(want, oracle.align(same, tb.scoring_with(sa, method, GAPS[method], asym()), triangular=True))  # letters of one code are one residue
    with context(sa, monkeypatch, store, scoring) as ctx:
        _, kernel = whole(ctx, store, want, f"{method} many-to-one lut")
        assert BUNDLE.match(kernel), kernel


@pytest.mark.parametrize("letters", ["BZX*", "*"])
@pytest.mark.parametrize("method", METHODS)
def test_codes_20_to_23_on_every_family(method, letters, sa, oracle, planner, monkeypatch):
    """the last real rows of every profile table, right below the SEP and NOP rows: stores made of the codes 20..23 only, and
    of code 23 only, 1..200 residues"""
    scoring = tb.scoring_with(sa, method, GAPS[method], asym())
    seqs = tb.random_sequences(list(range(1, 201)), 13, letters)
    assert {int(scoring.lut[ch]) for s in seqs for ch in s} == {tb.LETTERS24.index(ch) for ch in letters} <= {20, 21, 22, 23}
    store = sa.SequenceStore.from_sequences(seqs)
    lens = [len(s) for s in seqs]
    lim = planner(scoring, max(lens), min(lens))
    want = oracle.align(store, scoring, triangular=True, threads=16)
    for switch, family in ((None, None), ("SA_HIP_NO_SORT", None), ("SA_HIP_NO_PK", S32), ("SA_HIP_FORCE_GENERIC", GENERIC)):
        tag = f"{method} letters {letters} {switch or 'default'} limits {lim}"
        with context(sa, monkeypatch, store, scoring, switch) as ctx:
            _, kernel = whole(ctx, store, want, tag)
            if family:
                assert kernel.startswith(family), f"{tag}: {kernel}"
            else:
                assert "pk8" in check_forms(ctx, lens, lim, want, tag, every_form=False)


def test_letters_outside_the_table_are_refused(sa, oracle):
    scoring = tb.scoring_with(sa, "nw", GAPS["nw"], asym(), tb.lut_many())
    good = [b"ARNDjou.", b"wyvbzx*"]
    for letter in tb.REFUSED:
        with pytest.raises(sa.AlignError, match="Invalid character"):
            sa.hip_align(tb.raw_store(sa, good + [b"AR" + letter + b"N"]), scoring, triangular=True)
        with pytest.raises(sa.AlignError, match="Invalid character"):
            sa.Context(tb.raw_store(sa, [letter] + good), scoring, 0)
    store = tb.raw_store(sa, good)  # ... and the process lives on
    assert np.array_equal(sa.hip_align(store, scoring, triangular=True), oracle.align(store, scoring, triangular=True))
