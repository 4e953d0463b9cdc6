"""CPU: the oracle restatement and the option tables against the reference's own code -- live through
oracle/_ref/libseqalign_ref.so where /root/reference was present at build time, else against the answers that library
gave to the very same calls, stored by tools/make_golden.py (tests/golden/oracle_vs_ref.npz)."""
import json

import numpy as np
import pytest

from tests.oracle_binding import ROOT, RefLib, ref_available
from tests.synth import make_dna_set, make_protein_set

GOLDEN = ROOT / "tests" / "golden" / "oracle_vs_ref.npz"

CASES = [
    ("nw", "blosum62", dict(gap_pen=4)), ("nw", "pam120", dict(gap_pen=7)), ("ga", "blosum62", dict(gap_open=10, gap_extend=1)),
    ("ga", "blosum80", dict(gap_open=5, gap_extend=9)), ("sw", "blosum62", dict(gap_open=10, gap_extend=1)),
    ("sw", "blosum50", dict(gap_open=1, gap_extend=1)), ("ga", "blosum62", dict(gap_open=6, gap_extend=6)),
]


def case_key(method, matrix, gaps) -> str:
    return "_".join([method, matrix, *(f"{k}{v}" for k, v in sorted(gaps.items()))])


def random_store(sa):
    return sa.SequenceStore.from_sequences(make_protein_set(120, 1, 160, 31))


def dna_store(sa):
    return sa.SequenceStore.from_sequences(make_dna_set(80, 30, 200, 33, iupac=True))


def live_reference(method, matrix, gaps, store=None, full=False) -> dict:
    """the reference library's option tables and, for a store, its packed (and full) scores"""
    ref = RefLib(method, matrix, **gaps)
    try:
        p = ref.params()
        out = dict(lut=p["lut"], sub=p["sub"], method=np.array(p["method"]))
        if store is not None:
            out.update(blob=store.blob.copy(), meta=store.meta.copy(), tri=ref.align(store, triangular=True))
            if full:
                out["full"] = ref.align(store, triangular=False)
        return out
    finally:
        ref.close()


def reference(key, method, matrix, gaps, store=None, full=False) -> dict:
    if ref_available():
        return live_reference(method, matrix, gaps, store, full)
    with np.load(GOLDEN) as z:
        out = {name[len(key) + 1:]: z[name] for name in z.files if name.startswith(key + "/")}
    assert out, f"{GOLDEN.name} holds no entry {key}: regenerate it with tools/make_golden.py"
    assert json.loads(str(out.pop("gaps"))) == gaps
    if store is not None:  # (the stored answers belong to exactly this input)
        assert np.array_equal(out["blob"], store.blob) and np.array_equal(out["meta"], store.meta)
    return out


def stored_calls(sa):
    """every call whose answer GOLDEN keeps: (key, method, matrix, gaps, store, full)"""
    for method, matrix, gaps in CASES:
        yield case_key(method, matrix, gaps), method, matrix, gaps, random_store(sa), True
    for name in sa.matrix_names():
        yield f"matrix_{name}", "nw", name, dict(gap_pen=1), None, False
    yield "dna_sw_dnafull", "sw", "dnafull", dict(gap_open=16, gap_extend=4), dna_store(sa), False


@pytest.mark.parametrize("method,matrix,gaps", CASES)
def test_oracle_equals_reference_random(method, matrix, gaps, oracle, sa):
    store = random_store(sa)
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    p = reference(case_key(method, matrix, gaps), method, matrix, gaps, store, full=True)
    assert np.array_equal(p["lut"], scoring.lut) and np.array_equal(p["sub"], scoring.sub)
    assert str(p["method"]) == scoring.method_name
    assert np.array_equal(p["tri"], oracle.align(store, scoring, triangular=True))
    assert np.array_equal(p["full"], oracle.align(store, scoring, triangular=False))


def test_every_matrix_matches_reference(sa):
    for k, name in enumerate(sa.matrix_names()):
        kw = dict(gap_pen=1)
        p = reference(f"matrix_{name}", "nw", name, kw)
        s = sa.Scoring.from_names("nw", name, **kw)
        assert np.array_equal(p["lut"], s.lut), name
        assert np.array_equal(p["sub"], s.sub), name


def test_dna_and_filter(oracle, sa):
    store = dna_store(sa)
    scoring = sa.Scoring.from_names("sw", "dnafull", gap_open=16, gap_extend=4)
    p = reference("dna_sw_dnafull", "sw", "dnafull", dict(gap_open=16, gap_extend=4), store)
    assert np.array_equal(p["tri"], oracle.align(store, scoring, triangular=True))
