"""GPU (-m gpu): pre-built token streams of the packed kernels (sa_plan.cpp: sa_build_tokens; sa_systolic_pk.inc: the lean
block work) against the oracle AND against the same context built with SA_HIP_NO_TOKENS=1, in which every tile derives its
tokens from the code bytes as before.  SA_HIP_CHUNK makes full tiles small; ctx.token_tiles() says which way the tiles of
the last launch took, so that no case exercises the old way only: full tiles of an arranged level stream tokens, partial
tiles do not."""
import numpy as np
import pytest

from tests.synth import make_protein_set

pytestmark = pytest.mark.gpu

NW = ("nw", dict(gap_pen=4))
GA = ("ga", dict(gap_open=10, gap_extend=1))
SW = ("sw", dict(gap_open=10, gap_extend=1))


def tri(j):
    return j * (j - 1) // 2


def device_range(ctx, lo, n):
    import torch
    buf = torch.full((n + 8,), -77, dtype=torch.int32, device="cuda")
    ctx.align_range(lo, n, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[n:] == -77).all(), "wrote past the range"
    return out[:n]


def both_ways(sa, monkeypatch, store, scoring, chunk, ranges, want, need_legacy=False):
    """every range with token streams and without, against the oracle's scores and against each other"""
    monkeypatch.setenv("SA_HIP_CHUNK", str(chunk))  # (the switches are read when a context is created)
    got = {}
    for no_tokens in (False, True):
        if no_tokens:
            monkeypatch.setenv("SA_HIP_NO_TOKENS", "1")
        else:
            monkeypatch.delenv("SA_HIP_NO_TOKENS", raising=False)
        with sa.Context(store, scoring, 0) as ctx:
            for lo, n in ranges:
                got[no_tokens, lo, n] = device_range(ctx, lo, n)
                lean, legacy = ctx.token_tiles()
                if no_tokens:
                    assert lean == 0 and legacy >= 1, (lo, n, lean, legacy)
                else:
                    assert lean >= 1, f"range [{lo},+{n}): no tile streamed pre-built tokens ({legacy} derived them)"
                    assert legacy >= 1 or not need_legacy, f"range [{lo},+{n}): every tile streamed pre-built tokens"
    for lo, n in ranges:
        assert np.array_equal(got[False, lo, n], want[lo:lo + n]), f"range [{lo},+{n}) with token streams differs from the oracle"
        assert np.array_equal(got[True, lo, n], got[False, lo, n]), f"range [{lo},+{n}): SA_HIP_NO_TOKENS changes scores"


def scores(sa, oracle, seqs, method, gaps):
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    return store, scoring, oracle.align(store, scoring, triangular=True, threads=16)


@pytest.fixture(scope="module")
def nw101(sa, oracle):
    """32 m + r sequences (m = 3, r = 5) of 80-120 residues: with 32- and 64-row tiles the upper columns have full tiles
    and a partial one"""
    return scores(sa, oracle, make_protein_set(32 * 3 + 5, 80, 120, 41), *NW)


@pytest.mark.parametrize("chunk", [1, 2])
def test_full_and_partial_tiles_in_one_launch(chunk, nw101, sa, monkeypatch):
    store, scoring, want = nw101
    n = store.num
    ranges = [(0, store.pairs)] + [(tri(j), j) for j in (n - 1, n - 2, 70)]  # the whole range, and single columns
    both_ways(sa, monkeypatch, store, scoring, chunk, ranges, want, need_legacy=True)


def test_dense_terminator_masks(sa, oracle, monkeypatch):
    """rows of 1-8 residues (a terminator every 2-9 positions) in front of a few ~100-residue columns; 32 sequences per
    stream: the 1024 short rows are one full tile of the long columns"""
    seqs = make_protein_set(1024, 1, 8, 42) + make_protein_set(6, 95, 105, 43)
    store, scoring, want = scores(sa, oracle, seqs, *NW)
    lo = tri(1024)
    both_ways(sa, monkeypatch, store, scoring, 32, [(lo, store.pairs - lo), (0, store.pairs)], want)


def test_stream_lengths_around_multiples_of_16(sa, oracle, monkeypatch):
    """one sequence per stream, so a stream is len + 1 positions: 16 k - 1, 16 k and 16 k + 1 for k = 1, 2, 6; and a wave
    with streams of one 1-residue sequence beside streams of one 190-residue sequence (the first 32 rows: four of each are
    left over from the pure rounds and share the mixed round), many of whose blocks are all NOP"""
    base = make_protein_set(101, 190, 190, 44)
    lens = [190] * 4 + [1] * 4 + [50] * 8 + [60] * 8 + [70] * 8
    lens += [(14, 15, 16, 30, 31, 32, 94, 95, 96)[k % 9] for k in range(101 - len(lens))]
    store, scoring, want = scores(sa, oracle, [s[:l] for s, l in zip(base, lens)], *NW)
    both_ways(sa, monkeypatch, store, scoring, 1, [(0, store.pairs), (tri(100), 100), (tri(40), 40)], want)


@pytest.mark.parametrize("method,gaps", [GA, SW])
def test_gotoh_and_smith_waterman(method, gaps, sa, oracle, monkeypatch):
    store, scoring, want = scores(sa, oracle, make_protein_set(32 * 3 + 5, 60, 100, 45), method, gaps)
    both_ways(sa, monkeypatch, store, scoring, 2, [(0, store.pairs)], want, need_legacy=True)


def test_sixteen_lane_groups(sa, oracle, monkeypatch):
    """columns of 193-208 residues (K = 13) and of 641-656 (K = 41: tokens in units of 256 bytes) behind 70 rows of 30-60;
    16 streams of two sequences: the long columns have two full tiles and a partial one"""
    seqs = make_protein_set(70, 30, 60, 46) + make_protein_set(3, 194, 208, 47) + make_protein_set(3, 642, 656, 48)
    store, scoring, want = scores(sa, oracle, seqs, *NW)
    ranges = [(0, store.pairs), (tri(71), 71), (tri(75), 75)]
    both_ways(sa, monkeypatch, store, scoring, 2, ranges, want, need_legacy=True)


@pytest.fixture(scope="module")
def short2100(sa, oracle):
    return scores(sa, oracle, make_protein_set(2100, 5, 20, 49), *NW)


def test_tiles_smaller_than_their_arranged_block(short2100, sa, monkeypatch):
    """2100 short sequences in 256-row tiles, device output: the tiles stream the arranged blocks of 2048, 1024 and 512 rows,
    whose token streams are cut by stream, not by tile"""
    store, scoring, want = short2100
    lo, hi = tri(1500) + 17, tri(2090) - 5  # the whole range, and one cut inside columns at both ends
    both_ways(sa, monkeypatch, store, scoring, 8, [(0, store.pairs), (lo, hi - lo)], want, need_legacy=True)


def test_host_delivery(short2100, sa, monkeypatch):
    """the same store through the host-delivery loop into a page-locked matrix: a block is one tile, scores leave in row order"""
    store, scoring, want = short2100
    monkeypatch.setenv("SA_HIP_CHUNK", "8")
    dest = sa.PinnedMatrix(store.pairs)
    try:
        got = {}
        for no_tokens in (False, True):
            if no_tokens:
                monkeypatch.setenv("SA_HIP_NO_TOKENS", "1")
            else:
                monkeypatch.delenv("SA_HIP_NO_TOKENS", raising=False)
            with sa.Context(store, scoring, 0) as ctx:
                dest.array[:] = -77
                ctx.align_host(dest.array, triangular=True)
                got[no_tokens] = dest.array.copy()
                lean, legacy = ctx.token_tiles()  # (of the last batch of columns)
                assert (lean == 0) if no_tokens else (lean >= 1), (no_tokens, lean, legacy)
        assert np.array_equal(got[False], want)
        assert np.array_equal(got[True], got[False])
    finally:
        dest.close()


def placed_shares(ctx, pairs, world, elem16, host=None):
    """align_share of every rank of `world` over the whole range, then place_shares: (placed vector, lean, legacy summed over
    the ranks); guard words behind the shares and behind the placed vector"""
    import torch
    to_host = host is not None
    e = ctx.share_elems(0, pairs, world, to_host)
    shares = torch.full((world * e + 8,), -77, dtype=torch.int16 if elem16 else torch.int32, device="cuda")
    packed = torch.full((pairs + 8,), -77, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lean = legacy = 0
    for r in range(world):
        ctx.align_share(0, pairs, world, r, shares.data_ptr() + (2 if elem16 else 4) * r * e, elem16, st, host.ptr if to_host else 0)
        a, b = ctx.token_tiles()
        lean, legacy = lean + a, legacy + b
    ctx.place_shares(0, pairs, world, shares.data_ptr(), elem16, packed.data_ptr(), st, to_host)
    torch.cuda.synchronize()
    out = packed.cpu().numpy()
    assert (out[pairs:] == -77).all() and (shares[world * e:].cpu().numpy() == -77).all(), "wrote past the range"
    return out[:pairs], lean, legacy


@pytest.mark.parametrize("world", [2, 8])
def test_shares_of_two_tile_sizes(world, short2100, sa, monkeypatch):
    """the multi-rank path without SA_HIP_CHUNK: the planner cuts a rank's share into two tile sizes (chunk_pk and
    chunk_pk_small, each with arranged copies and token streams of its own: tests/test_plan_host.py has the plan); int16 and
    s32 elements, and for world 8 also with the scores going straight into a page-locked host matrix, where a block is one tile"""
    store, scoring, want = short2100
    monkeypatch.delenv("SA_HIP_CHUNK", raising=False)
    host = sa.PinnedMatrix(store.pairs) if world == 8 else None
    try:
        got = {}
        for no_tokens in (False, True):
            if no_tokens:
                monkeypatch.setenv("SA_HIP_NO_TOKENS", "1")
            else:
                monkeypatch.delenv("SA_HIP_NO_TOKENS", raising=False)
            with sa.Context(store, scoring, 0) as ctx:
                assert ctx.scores_fit16
                for elem16 in (True, False):
                    for dest in [None] + ([host] if host else []):
                        if dest:
                            dest.array[:] = -77
                        key = (elem16, dest is not None)
                        got[no_tokens, key], lean, legacy = placed_shares(ctx, store.pairs, world, elem16, dest)
                        assert (lean == 0 and legacy >= 1) if no_tokens else (lean >= 1), (no_tokens, key, lean, legacy)
                        assert not dest or np.array_equal(dest.array, want), f"world {world} {key} no_tokens {no_tokens}: host matrix differs from the oracle"
        for (no_tokens, key), v in got.items():
            assert np.array_equal(v, want), f"world {world} (int16, to_host) {key} no_tokens {no_tokens}: placed vector differs from the oracle"
            assert np.array_equal(v, got[False, key])
    finally:
        if host:
            host.close()
