"""GPU (-m gpu): the half and quarter tiles behind a column pair's last full tile (sa_shapes.h: sa_pk_piece_window;
sa_plan.cpp; the row window in pk_tile's prologue, sa_systolic_pk.inc) against the oracle AND, element for element, against
the same context built with SA_HIP_NO_REMAINDER=1, in which a pair's last rows are one store-order partial tile as before.

An all-vs-all store visits every remainder 0 .. tile_rows - 1 once its last column passes 2 x tile_rows, so SA_HIP_CHUNK
makes the tiles small: 512 rows (8-lane groups, chunk 16: half tiles of 256 rows, quarter tiles of 128) and 128 rows
(16-lane groups, chunk 8: half tiles of 64 rows, no quarter -- two sequences per stream are not on offer); one store fills a
bundle with all eight K, so that one launch walks main, half and quarter classes of each.  Every case goes
through device output, host delivery, a range cut inside columns, a bounded search context and the shares of worlds 2 and 3;
ctx.token_tiles() must show the lean count up by exactly the half and quarter tiles the rule gives for the store."""
import numpy as np
import pytest

from tests.synth import make_protein_set

pytestmark = pytest.mark.gpu

NW = ("nw", dict(gap_pen=4))
GA = ("ga", dict(gap_open=10, gap_extend=1))
SW = ("sw", dict(gap_open=10, gap_extend=1))

# name: (sequences, shortest, longest, seed, SA_HIP_CHUNK, lanes per group, rows of a full tile)
STORES = {
    "k3to5": (1100, 17, 40, 61, 16, 8, 512),     # K = 3..5: the row-stream classes of NW, the token ring for Gotoh and SW
    "k10to12": (1100, 73, 96, 62, 16, 8, 512),   # K = 10..12: the second profile row stride
    "lanes16": (300, 200, 260, 63, 8, 16, 128),  # 16-lane groups, K = 13..17
    "k1to8": (1100, 1, 64, 64, 16, 8, 512),      # a whole bundle: eight K x three variants = 24 classes in one launch
}
CASES = [("k3to5", NW), ("k3to5", GA), ("k3to5", SW), ("k10to12", NW), ("lanes16", NW), ("k1to8", NW)]
IDS = [f"{s}-{m[0]}" for s, m in CASES]


def tri(j):
    return j * (j - 1) // 2


def pieces_of(lens, method, chunk, g):
    """half and quarter tiles of the plan of the whole triangle, counted from the lengths by the rule alone: the columns of a
    class pair up in order, a pair's rows are [0, its last column), and what is left behind its full tiles is cut"""
    num = len(lens)
    cols = {}
    for j in range(1, num):
        k = (lens[j] + g - 1) // g
        assert (k <= 24) if g == 8 else (k >= 13 and (lens[j] + 7) // 8 > 24), "the store leaves the group width of its case"
        cols.setdefault(k, []).append(j)
    total = 0
    for k, js in cols.items():
        wpb = 8 if (g == 16 and k >= 45) or (method == "nw" and g == 8 and k >= 17) else 4
        rows = wpb * (64 // g) * chunk
        half = chunk % 2 == 0 and chunk // 2 >= 4 and rows // 2 <= num
        quarter = chunk % 4 == 0 and chunk // 4 >= 4 and rows // 4 <= num
        for c in range(0, len(js), 2):
            r = js[min(c + 1, len(js) - 1)] % rows
            if half and r >= rows // 2:
                total += 1
                r -= rows // 2
            if quarter:
                total += r // (rows // 4)
    return total


@pytest.fixture(scope="module")
def scored(sa, oracle):
    """store, scoring and the oracle's triangle of every case, computed once"""
    memo = {}

    def get(name, method):
        key = (name, method[0])
        if key not in memo:
            n, lo, hi, seed = STORES[name][:4]
            seqs = make_protein_set(n, lo, hi, seed)
            store = sa.SequenceStore.from_sequences(seqs)
            scoring = sa.Scoring.from_names(method[0], "blosum62", **method[1])
            want = oracle.align(store, scoring, triangular=True, threads=16)
            want.setflags(write=False)
            memo[key] = (seqs, store, scoring, want)
        return memo[key]
    return get


def both_plans(monkeypatch, chunk):
    """the two settings of the switch, in turn (a context reads it when it is created)"""
    monkeypatch.setenv("SA_HIP_CHUNK", str(chunk))
    for off in (False, True):
        if off:
            monkeypatch.setenv("SA_HIP_NO_REMAINDER", "1")
        else:
            monkeypatch.delenv("SA_HIP_NO_REMAINDER", raising=False)
        yield off


def device_range(ctx, lo, n):
    import torch
    buf = torch.full((n + 8,), -77, dtype=torch.int32, device="cuda")
    ctx.align_range(lo, n, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[n:] == -77).all(), "wrote past the range"
    return out[:n]


@pytest.mark.parametrize("name,method", CASES, ids=IDS)
def test_device_output_host_delivery_and_a_cut_range(name, method, scored, sa, monkeypatch):
    seqs, store, scoring, want = scored(name, method)
    chunk, g, rows = STORES[name][4:]
    assert store.num > 2 * rows, "the last column must pass two tiles: every remainder occurs"
    lo, hi = tri(store.num // 3) + 77, tri(store.num - 9) + store.num // 2  # starts and ends inside columns
    got, lean = {}, {}
    dest = sa.PinnedMatrix(store.pairs)
    try:
        for off in both_plans(monkeypatch, chunk):
            with sa.Context(store, scoring, 0) as ctx:
                got[off, "device"] = device_range(ctx, 0, store.pairs)
                lean[off], legacy = ctx.token_tiles()
                assert lean[off] >= 1 and legacy >= 1, (off, lean[off], legacy)  # (the residual partial tiles derive their tokens)
                got[off, "cut"] = device_range(ctx, lo, hi - lo)
                dest.array[:] = -77
                ctx.align_host(dest.array, triangular=True)
                got[off, "host"] = dest.array.copy()
    finally:
        dest.close()
    for way, ref in (("device", want), ("cut", want[lo:hi]), ("host", want)):
        assert np.array_equal(got[False, way], ref), f"{way}: remainder tiles differ from the oracle"
        assert np.array_equal(got[True, way], got[False, way]), f"{way}: SA_HIP_NO_REMAINDER changes scores"
    pieces = pieces_of([len(s) for s in seqs], method[0], chunk, g)
    assert pieces > store.num // 8, pieces  # (about three pairs in four have a half or a quarter tile)
    assert lean[False] - lean[True] == pieces, f"lean tiles {lean[True]} -> {lean[False]}, the rule gives {pieces} half and quarter tiles"


@pytest.mark.parametrize("name,method", CASES, ids=IDS)
def test_bounded_search_context(name, method, scored, sa, monkeypatch):
    """the database rows end a full tile, a half tile, a quarter of a tile and an eighth and two rows behind them: every
    query pair has a half tile, a quarter tile where the plan offers one, and a residual"""
    import torch
    seqs, store, scoring, want = scored(name, method)
    chunk, g, rows = STORES[name][4:]
    n_db = rows + rows // 2 + rows // 4 + rows // 8 + 2
    nq = store.num - n_db
    assert nq >= 8
    db, queries = sa.SequenceStore.from_sequences(seqs[:n_db]), sa.SequenceStore.from_sequences(seqs[n_db:])
    ref = np.stack([want[tri(n_db + q):tri(n_db + q) + n_db] for q in range(nq)])
    got, lean = {}, {}
    for off in both_plans(monkeypatch, chunk):
        with sa.SearchContext(db, queries, scoring, 0) as ctx:
            rect = torch.full((nq * n_db + 8,), -77, dtype=torch.int32, device="cuda")
            scratch = torch.empty(max(ctx.search_scratch_bytes(0, nq), 8), dtype=torch.uint8, device="cuda")
            ctx.search_range(0, nq, rect.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = rect.cpu().numpy()
            assert (out[nq * n_db:] == -77).all(), "wrote past the rectangle"
            got[off] = out[:nq * n_db].reshape(nq, n_db)
            lean[off] = ctx.token_tiles()[0]
    assert np.array_equal(got[False], ref), "remainder tiles differ from the oracle"
    assert np.array_equal(got[True], got[False]), "SA_HIP_NO_REMAINDER changes scores"
    assert lean[False] > lean[True], (lean[True], lean[False])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,method", CASES, ids=IDS)
def test_shares_of_emulated_ranks(name, method, world, scored, sa, monkeypatch):
    """every rank's share computed on this device in place of the all-gather: the placed vector and the host matrix the
    ranks stored into are the oracle's matrix, with and without remainder tiles"""
    import torch
    from sequencealigner_amd.distributed import HipShares, TiledGatherStep

    seqs, store, scoring, want = scored(name, method)
    chunk = STORES[name][4]
    host = sa.PinnedMatrix(store.pairs)
    got = {}
    try:
        for off in both_plans(monkeypatch, chunk):
            with sa.Context(store, scoring, 0) as ctx:
                for chunks, use16 in ((1, True), (2, False)):
                    host.array[:] = np.iinfo(np.int32).min
                    step = TiledGatherStep(HipShares(ctx, use16, host), store.num, world, world // 2, chunks, None)
                    step()
                    torch.cuda.synchronize()
                    got[off, chunks] = step.packed.cpu().numpy()
                    assert np.array_equal(host.array, want), (off, chunks, "host matrix")
    finally:
        host.close()
    for chunks in (1, 2):
        assert np.array_equal(got[False, chunks], want), f"{chunks} super-chunks: remainder tiles differ from the oracle"
        assert np.array_equal(got[True, chunks], got[False, chunks]), f"{chunks} super-chunks: SA_HIP_NO_REMAINDER changes scores"
