"""GPU (-m gpu): EVERY packed class and form on the lean way of pk_tile (sa_systolic_pk.inc: full tiles that stream the
pre-built tokens of an arranged level) against the oracle AND against the same context built with SA_HIP_NO_TOKENS=1.

The lean block work differs per instantiation: the scale of a token dword (TUNIT = PARTS 256 >> TSHIFT, TSHIFT = 8 from
K = 41), the 16-lane layout (one u16 per lane, the wave's mask at tk_any + (o_w >> 4) / NG), eight-wave workgroups (first
stream i_begin / chunk + wv NG with wv up to 7; NW 8-lane K >= 17 and 16-lane K >= 45), the two-way u16 form, Gotoh's lean
prologue.  tests/test_gpu_token_streams.py reaches a few 8-lane classes and NW at K = 13 and 41; the stores of the other
per-class tests are a few dozen rows, all partial tiles.  Here one store per bundle and method (tests/token_classes.py)
gives every class K three columns with tiles of each kind -- inside the 256-row arranged block, their own block, partial --
which tests/test_plan_host.py verifies from the planner without a device.  Every case

  * asks the planner for the limits of exactly its store (tests/planner_limits.py) and requires every class of the bundle to
    be admitted: nothing is skipped, nothing falls back to the s32 kernels;
  * compares the whole range np.array_equal with the oracle with and without token streams, and the two with each other;
  * runs every class as a range of its own (its three columns), compares it, and checks through ctx.timing that it ran
    sa_k_systolic_pk_bundle<method,G,KLO,form>[K k-k] with the lane width, bundle and form the limits give, and through
    ctx.token_tiles() that tiles took both ways with tokens on and none the lean way with tokens off;
  * checks the guard words behind every device range.

Oracle cost: the largest store (KLO = 53) is 3.7 x 10^4 residues, 7 x 10^8 cells; computed once per case at 16 threads."""
import numpy as np
import pytest

from tests import token_classes as tc
from tests.planner_limits import BUNDLE, class_of, form_of, planner  # noqa: F401  (planner: a fixture)
from tests.test_gpu_token_streams import device_range, tri
from tests.test_gpu_value_range import mismatch

pytestmark = pytest.mark.gpu

CASES = [pytest.param(g, klo, me, gaps, id=f"{me}-g{g}-klo{klo}") for g, klo in tc.BUNDLES for me, gaps in tc.METHODS]


def timed_range(ctx, lo, n):
    ctx.timing(True)
    got = device_range(ctx, lo, n)
    tm = ctx.timing_read()
    ctx.timing(False)
    return got, tm["kernel"]


def run_store(sa, oracle, planner, monkeypatch, g, klo, method, gaps, short_row=False):
    """the store of bundle (g, klo) both ways; returns (limits, {K: form is f16} of the classes that ran packed)"""
    seqs = tc.store_sequences(g, klo, short_row)
    lens = [len(s) for s in seqs]
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, tc.MATRIX, **gaps)
    lim = planner(scoring, max(lens), min(lens))
    assert lim["chunk_cap"] >= tc.CHUNK, lim
    packed = {}
    for k in tc.bundle_classes(g, klo):
        j = tc.first_column(g, klo, k, short_row)
        assert lens[j:j + 3] == tc.column_lengths(g, k)
        cls = {class_of(n, lim) for n in lens[j:j + 3]}
        if cls == {(g, k)}:
            packed[k] = form_of(g, k, lim)[1]
        else:  # only behind the last admitted class (the stores with a one-residue row; the caller says how far that may be)
            assert cls == {None} and k > lim["pk16"], f"{method} G {g} K {k}: columns of {lens[j:j + 3]} residues run as {cls} under {lim}"
    want = oracle.align(store, scoring, triangular=True, threads=16)
    monkeypatch.setenv("SA_HIP_CHUNK", str(tc.CHUNK))  # (the switches are read when a context is created)
    monkeypatch.delenv("SA_HIP_NO_SORT", raising=False)
    monkeypatch.delenv("SA_HIP_NO_PK", raising=False)
    whole, lean_of = {}, {}
    for no_tokens in (False, True):
        if no_tokens:
            monkeypatch.setenv("SA_HIP_NO_TOKENS", "1")
        else:
            monkeypatch.delenv("SA_HIP_NO_TOKENS", raising=False)
        way = "derived tokens (SA_HIP_NO_TOKENS)" if no_tokens else "token streams"
        with sa.Context(store, scoring, 0) as ctx:
            whole[no_tokens] = device_range(ctx, 0, store.pairs)
            lean, legacy = ctx.token_tiles()
            assert (lean == 0) if no_tokens else (lean >= 1 and legacy >= 1), (way, lean, legacy)
            for k, f16 in packed.items():
                j = tc.first_column(g, klo, k, short_row)
                lo, n = tri(j), tri(j + 3) - tri(j)
                tag = f"{method} G {g} K {k} ({'f16' if f16 else 'two-way u16'}), columns {j}..{j + 2}, {way}"
                got, kernel = timed_range(ctx, lo, n)
                lean, legacy = ctx.token_tiles()
                mt = BUNDLE.match(kernel)
                assert mt and (int(mt[1]), int(mt[2]), mt[3] == "true", int(mt[4]), int(mt[5])) == (g, klo, f16, k, k), f"{tag}: ran on {kernel}"
                if no_tokens:
                    assert lean == 0 and legacy >= 1, f"{tag}: {lean} lean, {legacy} legacy tiles"
                else:
                    assert lean >= 1, f"{tag}: no tile streamed pre-built tokens ({legacy} derived them)"
                    assert legacy >= 1, f"{tag}: every tile streamed pre-built tokens"
                    lean_of[k] = lean
                assert np.array_equal(got, want[lo:lo + n]), f"{tag}, {kernel}: " + mismatch(got, want[lo:lo + n], lo)
        assert np.array_equal(whole[no_tokens], want), f"{method} G {g} KLO {klo}, whole range, {way}: " + mismatch(whole[no_tokens], want)
    assert np.array_equal(whole[True], whole[False]), f"{method} G {g} KLO {klo}: SA_HIP_NO_TOKENS changes scores"
    assert set(lean_of) == set(packed)
    return lim, packed


@pytest.mark.parametrize("g,klo,method,gaps", CASES)
def test_every_class_of_a_bundle_on_the_lean_way(g, klo, method, gaps, sa, oracle, planner, monkeypatch):
    lim, packed = run_store(sa, oracle, planner, monkeypatch, g, klo, method, gaps)
    assert sorted(packed) == tc.bundle_classes(g, klo), f"{method} G {g} KLO {klo}: only K {sorted(packed)} are admitted under {lim}"


@pytest.mark.parametrize("method,gaps", tc.METHODS, ids=[me for me, _ in tc.METHODS])
def test_two_way_form_at_low_k(method, gaps, sa, oracle, planner, monkeypatch):
    """a one-residue row in front of the KLO = 13 and 21 stores: the frame shifts the bound then allows for move the low
    16-lane classes to the two-way u16 form, which otherwise starts at K = 53 (NW: every class, and none past K = 23)"""
    ran = {}
    for g, klo in tc.LOW_K_TWO_WAY:
        lim, packed = run_store(sa, oracle, planner, monkeypatch, g, klo, method, gaps, short_row=True)
        ran.update(packed)
    assert set(range(13, 24)) <= set(ran), f"{method}: of K = 13..23 only {sorted(ran)} ran packed"
    assert any(not f16 for f16 in ran.values()), f"{method}: no class ran the two-way form: {ran}"
