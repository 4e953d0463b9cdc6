"""GPU (-m gpu): the row-stream way of the packed NW kernels with 8-lane groups and K <= 16 (sa_plan.cpp:
sa_build_row_streams; sa_systolic_pk.inc: do_block's row-stream way) -- profile-row offsets loaded from global memory into
registers, sixteen per lane and block, no token ring.  Every case compares with the oracle AND with the same context built
with SA_HIP_NO_TOKENS=1 (every tile derives its tokens from the code bytes and goes through the ring), and asserts through
ctx.token_tiles() that lean tiles ran.  SA_HIP_CHUNK makes full tiles small."""
import numpy as np
import pytest

from tests.synth import make_protein_set

pytestmark = pytest.mark.gpu

NW = dict(gap_pen=4)


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


def both_ways(sa, monkeypatch, seqs, oracle, chunk, ranges=None, host=False, need_legacy=False):
    """the ranges (default: the whole matrix) with row streams and with SA_HIP_NO_TOKENS=1, against the oracle's scores and
    against each other; host: once more through align_host into a page-locked matrix"""
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names("nw", "blosum62", **NW)
    want = oracle.align(store, scoring, triangular=True, threads=16)
    ranges = ranges or [(0, store.pairs)]
    monkeypatch.setenv("SA_HIP_CHUNK", str(chunk))  # (the switches are read when a context is created)
    dest = sa.PinnedMatrix(store.pairs) if host else None
    try:
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
                        assert lean >= 1, f"range [{lo},+{n}): no tile streamed pre-built row offsets ({legacy} derived them)"
                        assert legacy >= 1 or not need_legacy, f"range [{lo},+{n}): every tile was a lean tile"
                if host:
                    dest.array[:] = -77
                    ctx.align_host(dest.array, triangular=True)
                    got[no_tokens, "host"] = dest.array.copy()
                    lean, legacy = ctx.token_tiles()  # (of the last batch of columns)
                    assert (lean == 0) if no_tokens else (lean >= 1), (no_tokens, lean, legacy)
        for lo, n in ranges:
            assert np.array_equal(got[False, lo, n], want[lo:lo + n]), f"range [{lo},+{n}) with row streams differs from the oracle"
            assert np.array_equal(got[True, lo, n], got[False, lo, n]), f"range [{lo},+{n}): SA_HIP_NO_TOKENS changes scores"
        if host:
            assert np.array_equal(got[False, "host"], want), "host delivery with row streams differs from the oracle"
            assert np.array_equal(got[True, "host"], got[False, "host"])
    finally:
        if dest:
            dest.close()


@pytest.mark.parametrize("steps", [16, 17, 32, 33])
def test_block_counts(steps, sa, oracle, monkeypatch):
    """chunk 1, one sequence per stream: a stream is len + 1 positions and a wave runs ceil((smax + 7) / 16) blocks.  Streams of
    steps - 7 positions make that 1, 2, 2 and 3 blocks -- an odd and an even number of two-block trips, the last step of a
    block taking its offset from the next block's registers -- and per 32 rows twelve 1-residue sequences sit beside twenty
    long ones: a wave of 1-residue streams only (one block), and a mixed wave whose short streams end on a terminator at
    position 1, inside the window that the later lanes of a group start at a negative position.  A few 100-residue columns
    behind them run the KLO = 9 bundle over the same rows."""
    long_len = steps - 7 - 1
    base = make_protein_set(32 * 3 + 4, 100, 100, 60 + steps)
    lens = [long_len if k % 32 < 20 else 1 for k in range(32 * 3)] + [100] * 4
    both_ways(sa, monkeypatch, [s[:l] for s, l in zip(base, lens)], oracle, 1, need_legacy=True)


@pytest.mark.parametrize("rows,cols", [((20, 40), ((89, 96), (97, 104))), ((5, 5), ((5, 5), (57, 64)))],
                         ids=["K12_K13_three_and_four_parts", "K1_K8_one_and_two_parts"])
def test_two_row_strides_in_one_launch(rows, cols, sa, oracle, monkeypatch):
    """columns of two classes whose profiles have different numbers of 16-byte parts, hence different row strides and
    different row-stream copies of the same arranged rows, in one bundle launch: K = 12 (96 columns) beside K = 13 (97-104) in
    the KLO = 9 bundle, K = 1 (5 residues) beside K = 8 (57-64) in the KLO = 1 bundle; 64 rows in front are two full tiles"""
    seqs = make_protein_set(64, rows[0], rows[1], 70)
    for k, (a, b) in enumerate(cols):
        seqs += make_protein_set(5, a, b, 71 + k)
    n = len(seqs)
    both_ways(sa, monkeypatch, seqs, oracle, 1, [(0, tri(n)), (tri(64), tri(n) - tri(64))], need_legacy=True)


def test_workgroups_that_run_lean_and_derived_tiles(sa, oracle, monkeypatch):
    """2100 sequences of 5-20 residues in 256-row tiles: more tiles than workgroup slots, so a persistent workgroup runs lean
    tiles (no ring) and derived tiles (partial: they clear and fill the ring themselves) one after the other; device output
    and the host-delivery loop, where a block is one tile and scores leave in row order"""
    both_ways(sa, monkeypatch, make_protein_set(2100, 5, 20, 72), oracle, 8, host=True, need_legacy=True)
