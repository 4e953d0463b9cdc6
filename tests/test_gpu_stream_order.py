"""GPU (-m gpu): the device-resident calls keep the order of their stream, queued and unsynchronised (include/seqalign_hip.h:
"asynchronous on `stream`", "no host synchronisation", "in order on one stream is fine").  tests/stream_order.py has the detector:
behind a calibrated delay on a side stream the true inputs are copied over decoys, the outputs are poisoned, the calls are issued
and the outputs are copied into snapshots -- the host waits for nothing in between.  Every expectation comes from the oracle and
from the references the other test files use, never from the code under test, and every element of every output buffer is
compared, the room behind a result included.

1. controls: a call handed another side stream, or stream 0, runs during the delay -- with the poison step its result is gone, without
   it the snapshot is exactly the expectation of the DECOY
2. every call that reads a device matrix or rectangle, once, truth over decoy
3. the calls whose inputs live in the context, and two pipelines chained without a host synchronisation
4. queued calls of one context: the counter ring used twice over by 520 single-column ranges of every kernel family, more distinct
   ranges than the plan cache holds, two contexts on two streams, one context on two streams as the header allows it"""
import types

import numpy as np
import pytest

from tests import agglo_ref
from tests.golden_util import tri_to_full
from tests.linkage_ref import prim_tree
from tests.search_cases import expected_hits, oracle_rect
from tests.stream_order import MIN_DELAY_MS, Detector, assert_differ, padded, poison_of
from tests.synth import AMINO20, make_protein_set
from tests.test_gpu_edges import expected_edges
from tests.test_gpu_identity import COLUMNS, pid_array, reference
from tests.test_gpu_neighbors import expected_neighbors
from tests.test_gpu_normalize import LENGTH, MAX, MIN, SELF, normalized, packed_ij
from tests.test_gpu_search_above import expected_csr
from tests.test_gpu_search_quantity import expected_values
from tests.test_gpu_select import expected_select

pytestmark = pytest.mark.gpu

N, PAIRS = 200, 19900
N_DB, M_Q = 130, 9
DELAY_MS = 200.0  # section 2 and 3: ample beside the first launch of a kernel, which loads its code object


def tri(j):
    return j * (j - 1) // 2


@pytest.fixture(scope="module")
def det():
    import torch
    d = Detector(torch)
    d.calibrate()
    print(f"\n[stream order] delay: {d.cycles_per_ms:.0f} cycles of torch.cuda._sleep per ms; asked for {MIN_DELAY_MS} ms, measured {d.measured_ms:.2f} ms")
    yield d
    print("\n[stream order] host time of the enqueues behind the delay, milliseconds (copies, poison, calls, snapshots):")
    for name, ms in d.enqueue_ms.items():
        print(f"[stream order]   {name:<40s} {ms:8.3f}")


@pytest.fixture(scope="module")
def streams(det):
    """two side streams, each used once for everything a case enqueues: the first use of a stream and of a fill or copy kernel takes
    milliseconds of host time, which belong to no case"""
    import torch
    made = torch.cuda.Stream(), torch.cuda.Stream()
    for s in made:
        with torch.cuda.stream(s):
            det.sleep(0.1)
            for dtype in (torch.int16, torch.int32, torch.int64):
                a = torch.zeros(64, dtype=dtype, device="cuda")
                a.fill_(1)
                torch.empty_like(a).copy_(a, non_blocking=True)
        s.synchronize()
    return made


@pytest.fixture(scope="module")
def w(sa, oracle):
    """200 proteins of 20 .. 60 residues; truth: their NW matrix, decoy: their Gotoh matrix"""
    seqs = make_protein_set(N, 20, 60, 77)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = {"T": sa.Scoring.from_names("nw", "blosum62", gap_pen=4), "D": sa.Scoring.from_names("ga", "blosum62", gap_open=10, gap_extend=1)}
    packed = {k: oracle.align(store, scoring[k], triangular=True) for k in "TD"}
    full = {k: tri_to_full(packed[k], N) for k in "TD"}
    lens = np.array([len(s) for s in seqs], np.int32)
    den = {"T": lens, "D": (lens[::-1] + 3).astype(np.int32)}  # (any N int32 are valid denominators)
    ctx = sa.Context(store, scoring["T"], 0)
    yield types.SimpleNamespace(seqs=seqs, store=store, scoring=scoring, packed=packed, full=full, den=den, lens=lens, ctx=ctx)
    ctx.close()


@pytest.fixture(scope="module")
def sw(sa, oracle):
    """130 database proteins, 9 queries; truth: the NW rectangle, decoy: the Gotoh rectangle"""
    db, queries = make_protein_set(N_DB, 20, 60, 78), make_protein_set(M_Q, 20, 60, 79)
    scoring = {"T": sa.Scoring.from_names("nw", "blosum62", gap_pen=4), "D": sa.Scoring.from_names("ga", "blosum62", gap_open=10, gap_extend=1)}
    rect = {k: oracle_rect(sa, oracle, db, queries, scoring[k]) for k in "TD"}
    lens = np.array([len(s) for s in db + queries], np.int32)
    den = {"T": lens, "D": (lens[::-1] + 3).astype(np.int32)}
    ctx = sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring["T"], 0)
    yield types.SimpleNamespace(db=db, queries=queries, scoring=scoring, rect=rect, den=den, ctx=ctx)
    ctx.close()


class Case:
    """inputs: (truth, decoy) host arrays per device input; outputs: (dtype, elements) per device output; want: {"T": [...], "D":
    [...]} the expectation of every output (shorter than its buffer: POISON stays behind it); enqueue(ins, outs, scratch, stream)
    with device pointers; scratch: bytes per scratch buffer; warm: one synchronised call first (a plan, a first allocation)"""

    def __init__(self, name, inputs, outputs, want, enqueue, scratch=(), warm=False):
        self.name, self.inputs, self.outputs, self.want, self.enqueue, self.scratch, self.warm = name, inputs, outputs, want, enqueue, scratch, warm


TORCH_OF = {np.dtype(np.int32): "int32", np.dtype(np.int64): "int64", np.dtype(np.int16): "int16"}


def execute(det, stream, case, call_stream=None, poison=True, delay_ms=DELAY_MS, name=None):
    torch = det.torch
    ins = []
    for t, d in case.inputs:
        assert t.shape == d.shape and t.dtype == d.dtype
        dt, dd = torch.from_numpy(np.ascontiguousarray(t)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
        ins.append((torch.empty_like(dt), dt, dd))
    outs = [torch.empty(size, dtype=getattr(torch, TORCH_OF[np.dtype(dt)]), device="cuda") for dt, size in case.outputs]
    scratch = [torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device="cuda") for nbytes in case.scratch]

    def enqueue(s):
        case.enqueue([b.data_ptr() for b, _, _ in ins], [o.data_ptr() for o in outs], [x.data_ptr() for x in scratch], s)
    if case.warm:
        for buf, truth, _ in ins:
            buf.copy_(truth)
        torch.cuda.synchronize()
        enqueue(stream.cuda_stream)
        torch.cuda.synchronize()
    return det.run(stream, ins, outs, enqueue, call_stream=call_stream, poison=poison, delay_ms=delay_ms, name=name)


def same(what, snaps, want):
    """every element of every output buffer: the expectation, then POISON"""
    assert len(snaps) == len(want)
    for k, (g, x) in enumerate(zip(snaps, want)):
        x = padded(np.asarray(x), g.size)
        assert g.dtype == x.dtype, f"{what}: output {k} is {g.dtype}, want {x.dtype}"
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, f"{what}: {bad.size} of {x.size} elements of output {k} differ, first at {bad[0]}: got {g[bad[0]]}, want {x[bad[0]]}"


def keeps_order(det, stream, case, unsynced=True):
    """the case twice -- the first run may meet a kernel's first launch, the second gives the enqueue time that is recorded"""
    if case.inputs:
        assert_differ(case.name, case.want["T"], case.want["D"])
    for name in (None, case.name):
        run = execute(det, stream, case, name=name)
        same(case.name, run.snaps, case.want["T"])
        det.check(run, case.name, unsynced)


# ---- the calls that read a device matrix or rectangle ----------------------------------------------------------------------------
K_NEIGHBORS, K_HITS = 7, 5
RANKS = [0, PAIRS // 100, PAIRS // 2, PAIRS - 1]


def flat_tree(tree):
    pairs, score = tree
    return [pairs.reshape(-1), score]


def matrix_case(name, sa, w):
    ctx, i32, i64 = w.ctx, np.int32, np.int64
    both = lambda f: {k: f(k) for k in "TD"}  # noqa: E731
    matrix = [(w.packed["T"], w.packed["D"])]
    if name == "neighbors":
        return Case(name, matrix, [(i32, N * K_NEIGHBORS)] * 2, both(lambda k: [a.reshape(-1) for a in expected_neighbors(w.full[k], K_NEIGHBORS)]),
                    lambda i, o, x, s: ctx.neighbors(i[0], K_NEIGHBORS, o[0], o[1], stream=s), warm=True)
    if name == "edges":  # offsets, then fill, with nothing in between; the buffers hold the N (N - 1) entries of the worst case
        t = int(np.sort(w.packed["T"])[int(0.9 * PAIRS)])

        def enqueue(i, o, x, s):
            ctx.edge_offsets(i[0], t, o[0], stream=s)
            ctx.edge_fill(i[0], t, o[0], o[1], o[2], stream=s)
        return Case(name, matrix, [(i64, N + 1), (i32, N * (N - 1)), (i32, N * (N - 1))], both(lambda k: list(expected_edges(w.full[k].copy(), t))), enqueue)
    if name == "linkage":
        return Case(name, matrix, [(i32, 2 * (N - 1)), (i32, N - 1)], both(lambda k: flat_tree(prim_tree(w.full[k]))),
                    lambda i, o, x, s: ctx.linkage(i[0], o[0], o[1], x[0], stream=s), scratch=[sa.linkage_scratch_bytes(N)])
    if name in ("agglomerate-complete", "agglomerate-average"):
        method = agglo_ref.METHODS[name.split("-")[1]]
        return Case(name, matrix, [(i32, 2 * (N - 1)), (i32, N - 1)], both(lambda k: flat_tree(agglo_ref.agglo_numpy(w.full[k], method))),
                    lambda i, o, x, s: ctx.agglomerate(i[0], method, o[0], o[1], x[0], stream=s), scratch=[sa.agglo_scratch_bytes(N, method)])
    if name == "select":
        return Case(name, matrix, [(i32, len(RANKS)), (i64, len(RANKS))], both(lambda k: list(expected_select(np.sort(w.packed[k]), RANKS))),
                    lambda i, o, x, s: ctx.select(i[0], RANKS, o[0], o[1], x[0], stream=s), scratch=[sa.select_scratch_bytes(len(RANKS))])
    if name == "normalize":
        pi, pj = packed_ij(N)
        return Case(name, matrix + [(w.den["T"], w.den["D"])], [(i32, PAIRS)], both(lambda k: [normalized(w.packed[k], w.den[k][pi], w.den[k][pj], MAX)]),
                    lambda i, o, x, s: ctx.normalize(i[0], i[1], MAX, o[0], stream=s))
    if name == "expand_full":
        return Case(name, matrix, [(i32, N * N)], both(lambda k: [w.full[k].reshape(-1)]), lambda i, o, x, s: ctx.expand_full(i[0], o[0], stream=s), warm=True)
    if name == "widen16":
        assert all(np.abs(w.packed[k]).max() < 2 ** 15 for k in "TD")
        return Case(name, [(w.packed["T"].astype(np.int16), w.packed["D"].astype(np.int16))], [(i32, PAIRS)], both(lambda k: [w.packed[k]]),
                    lambda i, o, x, s: ctx.widen16(i[0], o[0], PAIRS, stream=s), warm=True)
    raise KeyError(name)


MATRIX_CALLS = ["neighbors", "edges", "linkage", "agglomerate-complete", "agglomerate-average", "select", "normalize", "expand_full", "widen16"]


def rect_case(name, sa, sw):
    ctx, i32, i64 = sw.ctx, np.int32, np.int64
    both = lambda f: {k: f(k) for k in "TD"}  # noqa: E731
    rect = [(sw.rect["T"], sw.rect["D"])]
    if name == "hits":
        return Case(name, rect, [(i32, M_Q * K_HITS)] * 2, both(lambda k: [a.reshape(-1) for a in expected_hits(sw.rect[k], K_HITS)]),
                    lambda i, o, x, s: ctx.hits(i[0], M_Q, K_HITS, o[0], o[1], x[0], stream=s), scratch=[sa.hits_scratch_bytes(N_DB, M_Q, K_HITS)], warm=True)
    if name == "hits_take":  # the indices are a device input too: the hits of each rectangle, whose raw scores are then their scores
        index = both(lambda k: expected_hits(sw.rect[k], K_HITS)[0])
        return Case(name, rect + [(index["T"], index["D"])], [(i32, M_Q * K_HITS)], both(lambda k: [expected_hits(sw.rect[k], K_HITS)[1].reshape(-1)]),
                    lambda i, o, x, s: ctx.hits_take(i[0], M_Q, K_HITS, i[1], o[0], stream=s), warm=True)
    if name == "normalize_rect":
        return Case(name, rect + [(sw.den["T"], sw.den["D"])], [(i32, M_Q * N_DB)], both(lambda k: [expected_values(sw.rect[k], sw.den[k], N_DB, 0, MIN).reshape(-1)]),
                    lambda i, o, x, s: ctx.normalize_rect(i[0], M_Q, 0, i[1], MIN, o[0], stream=s))
    if name == "hits_above":  # offsets, then fill; value = score = the rectangle itself; nq * N entries of room
        t = int(np.sort(sw.rect["T"].reshape(-1))[int(0.8 * M_Q * N_DB)])

        def enqueue(i, o, x, s):
            ctx.hits_above_offsets(i[0], M_Q, t, o[0], x[0], stream=s)
            ctx.hits_above_fill(i[0], i[0], M_Q, t, o[0], x[0], o[1], o[2], o[3], stream=s)
        return Case(name, rect, [(i64, M_Q + 1)] + [(i32, M_Q * N_DB)] * 3, both(lambda k: list(expected_csr(sw.rect[k], sw.rect[k], t))), enqueue,
                    scratch=[sa.hits_above_scratch_bytes(N_DB, M_Q)])
    raise KeyError(name)


RECT_CALLS = ["hits", "hits_take", "normalize_rect", "hits_above"]


# ---- 1. controls: the detector sees a call on the wrong stream ------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [True, False], ids=["poisoned", "unpoisoned"])
@pytest.mark.parametrize("where", ["second side stream", "stream 0"])
@pytest.mark.parametrize("name", ["neighbors", "hits_above"])
def test_control_a_call_on_another_stream_is_seen(name, where, poison, det, streams, sa, w, sw):
    """a caller's error with valid inputs: the call runs while the delay holds S back, so it reads the decoy.  With the poison step
    its result is overwritten before the snapshot; without it the snapshot is the decoy's expectation, element for element."""
    import torch
    case = matrix_case(name, sa, w) if name in MATRIX_CALLS else rect_case(name, sa, sw)
    case.warm = True
    assert_differ(name, case.want["T"], case.want["D"])
    other = streams[1] if where == "second side stream" else torch.cuda.default_stream()
    run = execute(det, streams[0], case, call_stream=other, poison=poison, delay_ms=MIN_DELAY_MS)
    det.check(run, f"control {name} on {where}")
    same(f"control {name} on {where}", run.snaps, [np.zeros(0, g.dtype) for g in run.snaps] if poison else case.want["D"])


# ---- 2. every call that reads a device matrix or rectangle ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRIX_CALLS)
def test_matrix_call_keeps_stream_order(name, det, streams, sa, w):
    keeps_order(det, streams[0], matrix_case(name, sa, w))


@pytest.mark.parametrize("name", RECT_CALLS)
def test_rectangle_call_keeps_stream_order(name, det, streams, sa, sw):
    keeps_order(det, streams[0], rect_case(name, sa, sw))


def test_place_shares_keeps_stream_order(det, streams, sa, w):
    """the gathered shares of two ranks are a device input in tile order.  Where pair p sits in them is read once from the placement of
    a vector of indices (synchronised, before the case): truth and decoy are then the two oracle matrices laid out that way, and
    the expectation of the placement is the oracle matrix itself"""
    import torch
    world, ctx = 2, w.ctx
    e = ctx.share_elems(0, PAIRS, world)
    assert world * e >= PAIRS
    d_iota, d_at = torch.arange(world * e, dtype=torch.int32, device="cuda"), torch.full((PAIRS,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.place_shares(0, PAIRS, world, d_iota.data_ptr(), False, d_at.data_ptr())
    torch.cuda.synchronize()
    at = d_at.cpu().numpy()
    assert at.min() >= 0 and at.max() < world * e and np.unique(at).size == PAIRS, "the placement of an index vector is not a permutation into the shares"
    shares = {}
    for k in "TD":
        shares[k] = np.full(world * e, 12345, np.int32)
        shares[k][at] = w.packed[k]
    case = Case("place_shares", [(shares["T"], shares["D"])], [(np.int32, PAIRS)], {k: [w.packed[k]] for k in "TD"},
                lambda i, o, x, s: ctx.place_shares(0, PAIRS, world, i[0], False, o[0], stream=s), warm=True)
    keeps_order(det, streams[0], case)


# ---- 3. the calls whose inputs live in the context ------------------------------------------------------------------------------------
ID_START, ID_COUNT = tri(150) + 37, 300  # begins and ends inside a column
RECT_Q0, RECT_NQ = 3, 2


def context_case(name, sa, oracle, w, sw):
    i32 = np.int32
    ctx, sctx = w.ctx, sw.ctx
    only = lambda *arrays: {"T": list(arrays)}  # noqa: E731
    if name == "align_range":
        return Case(name, [], [(i32, PAIRS)], only(w.packed["T"]), lambda i, o, x, s: ctx.align_range(0, PAIRS, o[0], stream=s), warm=True)
    if name == "align_range16":
        return Case(name, [], [(np.int16, PAIRS)], only(w.packed["T"].astype(np.int16)), lambda i, o, x, s: ctx.align_range16(0, PAIRS, o[0], stream=s), warm=True)
    if name == "align_share":  # the shares of both ranks, then their placement: the share layout itself has no reference
        e = ctx.share_elems(0, PAIRS, 2)

        def enqueue(i, o, x, s):
            for r in range(2):
                ctx.align_share(0, PAIRS, 2, r, x[0] + 4 * r * e, False, stream=s)
            ctx.place_shares(0, PAIRS, 2, x[0], False, o[0], stream=s)
        return Case(name, [], [(i32, PAIRS)], only(w.packed["T"]), enqueue, scratch=[4 * 2 * e], warm=True)
    if name == "identity_range":
        pairs = [(int(i), int(j)) for i, j in zip(*packed_ij(N))][ID_START:ID_START + ID_COUNT]
        score, ident, cols, _ = reference(w.scoring["T"], w.seqs, pairs)
        assert np.array_equal(score, w.packed["T"][ID_START:ID_START + ID_COUNT])
        return Case(name, [], [(i32, ID_COUNT)] * 4, only(score, ident, cols, pid_array(ident, cols, w.lens.tolist(), pairs, COLUMNS)),
                    lambda i, o, x, s: ctx.identity_range(ID_START, ID_COUNT, score=o[0], identities=o[1], columns=o[2], pid=o[3], denom=COLUMNS, stream=s), warm=True)
    if name in ("denominators-self", "denominators-length"):
        want = np.array([oracle.pair(w.scoring["T"], q, q) for q in w.seqs], i32) if name.endswith("self") else w.lens
        source = SELF if name.endswith("self") else LENGTH
        return Case(name, [], [(i32, N)], only(want), lambda i, o, x, s: ctx.denominators(source, o[0], stream=s), warm=True)
    if name == "search_range":
        return Case(name, [], [(i32, M_Q * N_DB)], only(sw.rect["T"].reshape(-1)), lambda i, o, x, s: sctx.search_range(0, M_Q, o[0], x[0], stream=s),
                    scratch=[sctx.search_scratch_bytes(0, M_Q)], warm=True)
    if name == "identity_rect":
        cat = sw.db + sw.queries
        pairs = [(d, N_DB + q) for q in range(RECT_Q0, RECT_Q0 + RECT_NQ) for d in range(N_DB)]
        score, ident, cols, _ = reference(sw.scoring["T"], cat, pairs)
        assert np.array_equal(score, sw.rect["T"][RECT_Q0:RECT_Q0 + RECT_NQ].reshape(-1))
        return Case(name, [], [(i32, RECT_NQ * N_DB)] * 4, only(score, ident, cols, pid_array(ident, cols, [len(q) for q in cat], pairs, COLUMNS)),
                    lambda i, o, x, s: sctx.identity_rect(RECT_Q0, RECT_NQ, score=o[0], identities=o[1], columns=o[2], pid=o[3], denom=COLUMNS, stream=s), warm=True)
    raise KeyError(name)


CONTEXT_CALLS = ["align_range", "align_range16", "align_share", "identity_range", "denominators-self", "denominators-length", "search_range", "identity_rect"]


@pytest.mark.parametrize("name", CONTEXT_CALLS)
def test_context_call_keeps_stream_order(name, det, streams, sa, oracle, w, sw):
    keeps_order(det, streams[0], context_case(name, sa, oracle, w, sw))


def test_pipeline_align_normalize_neighbors(det, streams, sa, w):
    """each link reads what the link before it wrote; the denominators are the one device input, truth over decoy"""
    ctx = w.ctx
    pi, pj = packed_ij(N)
    want = {}
    for k in "TD":  # (the decoy's expectation: the true scores under the decoy denominators)
        values = normalized(w.packed["T"], w.den[k][pi], w.den[k][pj], MIN)
        want[k] = [w.packed["T"], values] + [a.reshape(-1) for a in expected_neighbors(tri_to_full(values, N), K_NEIGHBORS)]
    assert_differ("align -> normalize -> neighbors", want["T"][1:], want["D"][1:])

    def enqueue(i, o, x, s):
        ctx.align_range(0, PAIRS, o[0], stream=s)
        ctx.normalize(o[0], i[0], MIN, o[1], stream=s)
        ctx.neighbors(o[1], K_NEIGHBORS, o[2], o[3], stream=s)
    case = Case("align_range -> normalize -> neighbors", [(w.den["T"], w.den["D"])], [(np.int32, PAIRS)] * 2 + [(np.int32, N * K_NEIGHBORS)] * 2, want, enqueue, warm=True)
    for name in (None, case.name):
        run = execute(det, streams[0], case, name=name)
        same(case.name, run.snaps, want["T"])
        det.check(run, case.name)


def test_pipeline_search_normalize_hits_take(det, streams, sa, sw):
    ctx = sw.ctx
    want = {}
    for k in "TD":
        values = expected_values(sw.rect["T"], sw.den[k], N_DB, 0, MAX)
        index, value = expected_hits(values, K_HITS)
        want[k] = [sw.rect["T"].reshape(-1), values.reshape(-1), index.reshape(-1), value.reshape(-1), np.take_along_axis(sw.rect["T"], index.astype(np.int64), 1).reshape(-1)]
    assert_differ("search -> normalize_rect -> hits -> hits_take", want["T"][1:], want["D"][1:])

    def enqueue(i, o, x, s):
        ctx.search_range(0, M_Q, o[0], x[0], stream=s)
        ctx.normalize_rect(o[0], M_Q, 0, i[0], MAX, o[1], stream=s)
        ctx.hits(o[1], M_Q, K_HITS, o[2], o[3], x[1], stream=s)
        ctx.hits_take(o[0], M_Q, K_HITS, o[2], o[4], stream=s)
    case = Case("search_range -> normalize_rect -> hits -> hits_take", [(sw.den["T"], sw.den["D"])], [(np.int32, M_Q * N_DB)] * 2 + [(np.int32, M_Q * K_HITS)] * 3,
                want, enqueue, scratch=[ctx.search_scratch_bytes(0, M_Q), sa.hits_scratch_bytes(N_DB, M_Q, K_HITS)], warm=True)
    for name in (None, case.name):
        run = execute(det, streams[0], case, name=name)
        same(case.name, run.snaps, want["T"])
        det.check(run, case.name)


# ---- 4. queued calls of one context ---------------------------------------------------------------------------------------------------
def family_sequences():
    """70 sequences of 20 .. 60 residues, 6 of 200 .. 260, 4 of 1030 .. 1500, dealt so that neighbouring columns differ in kind"""
    rng = np.random.default_rng(4242)
    lens = rng.integers(20, 61, 70).tolist() + rng.integers(200, 261, 6).tolist() + rng.integers(1030, 1501, 4).tolist()
    order = np.argsort([(k * 7) % 80 for k in range(80)], kind="stable")  # (7 and 80 are coprime: a permutation)
    a = np.frombuffer(AMINO20, np.uint8)
    return [a[rng.integers(0, 20, int(lens[k]))].tobytes() for k in order]


FAMILIES = {  # context -> (environment, scoring, what the dominant kernel of a column must be named for its length)
    "packed": ({}, dict(gap_pen=4), {(20, 60): "sa_k_systolic_pk_bundle<nw,8,", (200, 260): "sa_k_systolic_pk_bundle<nw,16,", (1030, 1500): "sa_k_systolic<nw,G64,K16,strips>"}),
    "s32": ({"SA_HIP_NO_PK": "1"}, dict(gap_pen=4), {(20, 60): "sa_k_systolic<nw,G", (200, 260): "sa_k_systolic", (1030, 1500): "sa_k_systolic<nw,G64,K16,strips>"}),
    "pair-per-wave": ({}, dict(gap_pen=300), {(20, 60): "sa_k_pair_per_wave<nw>", (200, 260): "sa_k_pair_per_wave<nw>", (1030, 1500): "sa_k_pair_per_wave<nw>"}),
}


@pytest.fixture(scope="module")
def fam(sa, oracle):
    import os
    import torch
    seqs = family_sequences()
    store = sa.SequenceStore.from_sequences(seqs)
    lens = [len(s) for s in seqs]
    made = {}
    for key, (env, gaps, kernels) in FAMILIES.items():
        scoring = sa.Scoring.from_names("nw", "blosum62", **gaps)
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)  # (a context reads the switches when it is created)
        try:
            ctx = sa.Context(store, scoring, 0)
        finally:
            for k, v in old.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        want = oracle.align(store, scoring, triangular=True)
        # the family of each kind of column, through the timing of a separate, synchronised call (timing stays off afterwards)
        for (low, top), prefix in kernels.items():
            j = max(c for c in range(1, len(seqs)) if low <= lens[c] <= top)
            buf = torch.empty(j, dtype=torch.int32, device="cuda")
            ctx.timing(True)
            ctx.align_range(tri(j), j, buf.data_ptr())
            torch.cuda.synchronize()
            kernel = ctx.timing_read()["kernel"]
            ctx.timing(False)
            assert kernel.startswith(prefix), f"{key}: column {j} ({lens[j]} residues) ran on {kernel}, not on {prefix}..."
            assert np.array_equal(buf.cpu().numpy(), want[tri(j):tri(j + 1)])
        made[key] = types.SimpleNamespace(ctx=ctx, want=want, scoring=scoring)
    yield types.SimpleNamespace(seqs=seqs, store=store, lens=lens, n=len(seqs), **made)
    for v in made.values():
        v.ctx.close()


def queued(det, stream, ctx, want, ranges, identity_every=0, delay_ms=DELAY_MS, name=None):
    """every range of `ranges` into a place of its own of one output, behind one delay; every identity_every-th range also as
    sa_ctx_identity_range (scores only) into a second output.  Returns the run and the two expectations."""
    torch = det.torch
    at = np.concatenate([[0], np.cumsum([c for _, c in ranges])]).astype(np.int64)
    ident = [k for k in range(len(ranges)) if identity_every and k % identity_every == 0]
    iat = np.concatenate([[0], np.cumsum([ranges[k][1] for k in ident])]).astype(np.int64)
    outs = [torch.empty(int(at[-1]), dtype=torch.int32, device="cuda"), torch.empty(max(int(iat[-1]), 1), dtype=torch.int32, device="cuda")]

    def enqueue(s):
        nth = 0
        for k, (lo, cnt) in enumerate(ranges):
            ctx.align_range(lo, cnt, outs[0].data_ptr() + 4 * int(at[k]), stream=s)
            if nth < len(ident) and ident[nth] == k:
                ctx.identity_range(lo, cnt, score=outs[1].data_ptr() + 4 * int(iat[nth]), stream=s)
                nth += 1
    run = det.run(stream, [], outs, enqueue, delay_ms=delay_ms, name=name)
    return run, [np.concatenate([want[lo:lo + c] for lo, c in ranges]), np.concatenate([want[ranges[k][0]:ranges[k][0] + ranges[k][1]] for k in ident] + [np.zeros(0, np.int32)])]


@pytest.mark.parametrize("key", list(FAMILIES))
def test_counter_ring_twice_over(key, det, streams, fam):
    """520 single-column ranges of one context behind one delay: each of its 256 counter slots is taken a second time while its first
    user is still queued; neighbouring columns run on different kernels, and strip-mined, pair-per-wave and identity launches
    follow each other on the context's scratch.  79 distinct ranges: no plan is evicted, and all are cached by a first pass."""
    import torch
    c = getattr(fam, key)
    columns = [(tri(j), j) for j in range(1, fam.n)]
    assert len(columns) <= 100
    for lo, cnt in columns:  # (plans, arranged copies, the strip-mined scratch, the identity payloads)
        buf = torch.empty(cnt, dtype=torch.int32, device="cuda")
        c.ctx.align_range(lo, cnt, buf.data_ptr())
    c.ctx.identity_range(0, 1, score=buf.data_ptr())
    torch.cuda.synchronize()
    ranges = [columns[(11 * k) % len(columns)] for k in range(520)]
    run, want = queued(det, streams[0], c.ctx, c.want, ranges, identity_every=13, delay_ms=1500.0, name=f"520 align_range + 40 identity_range, {key}")
    same(f"ring, {key}", run.snaps, want)
    det.check(run, f"ring, {key}")


def test_more_ranges_than_the_plan_cache_holds(det, streams, fam):
    """170 distinct ranges in one go: once the context holds 160 plans the least recently used is evicted for every new one, and its
    device tables are freed while the launch that reads them is still queued behind the delay.  hipFree is documented to synchronise the device (hip_runtime_api.h:
    "performs an implicit hipDeviceSynchronize() call"), which is what the code relies on: the host waits there, so the stream may be
    idle afterwards and only the values are asserted."""
    c = fam.packed
    ranges = []
    for j in range(fam.n - 1, 2, -1):
        ranges += [(tri(j), j), (tri(j), j // 2), (tri(j) + j // 2, j - j // 2)]
    ranges = ranges[:170]
    assert len(set(ranges)) == 170
    run, want = queued(det, streams[0], c.ctx, c.want, ranges, name="170 distinct ranges (plans built, ten or more evicted)")
    same("eviction", run.snaps, want)


def two_streams(det, streams, jobs, delay_ms=DELAY_MS):
    """jobs: per stream (ctx, want, ranges); a delay on each stream, then poison, calls alternating between the streams, snapshots"""
    import time
    torch = det.torch
    outs, ats = [], []
    for _, _, ranges in jobs:
        at = np.concatenate([[0], np.cumsum([c for _, c in ranges])]).astype(np.int64)
        ats.append(at)
        outs.append(torch.full((int(at[-1]),), poison_of(np.int32), dtype=torch.int32, device="cuda"))
    snaps = [torch.zeros_like(o) for o in outs]
    torch.cuda.synchronize()
    marks = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in streams]
    for s, (began, ended) in zip(streams, marks):
        with torch.cuda.stream(s):
            began.record(s)
            det.sleep(delay_ms)
            ended.record(s)
    t0 = time.perf_counter()
    for s, o in zip(streams, outs):
        with torch.cuda.stream(s):
            o.fill_(poison_of(np.int32))
    for k in range(max(len(r) for _, _, r in jobs)):
        for s, (ctx, _, ranges), o, at in zip(streams, jobs, outs, ats):
            if k < len(ranges):
                ctx.align_range(ranges[k][0], ranges[k][1], o.data_ptr() + 4 * int(at[k]), stream=s.cuda_stream)
    for s, o, snap in zip(streams, outs, snaps):
        with torch.cuda.stream(s):
            snap.copy_(o, non_blocking=True)
    host_ms = (time.perf_counter() - t0) * 1e3
    idle = [bool(s.query()) for s in streams]
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    lasted = min(a.elapsed_time(b) for a, b in marks)
    assert lasted >= MIN_DELAY_MS and lasted >= 10 * host_ms, f"the enqueues took {host_ms:.3f} ms behind delays of {lasted:.2f} ms"
    assert not any(idle), f"a stream was idle when the last enqueue returned: {idle}"
    for snap, (_, want, ranges) in zip(snaps, jobs):
        same("two streams", [snap.cpu().numpy()], [np.concatenate([want[lo:lo + c] for lo, c in ranges])])
    return host_ms


def column_blocks(n, parts):
    cuts = [1 + (n - 1) * k // parts for k in range(parts + 1)]
    return [(tri(a), tri(b) - tri(a)) for a, b in zip(cuts[:-1], cuts[1:])]


def test_two_contexts_on_two_streams(det, streams, sa, w, fam):
    """different stores and methods: the mixed-length store under NW on one stream, the 200 proteins under Gotoh on the other"""
    import torch
    with sa.Context(w.store, w.scoring["D"], 0) as gotoh:
        jobs = [(fam.packed.ctx, fam.packed.want, column_blocks(fam.n, 6)), (gotoh, w.packed["D"], column_blocks(N, 6))]
        for ctx, _, ranges in jobs:  # (plans and first allocations)
            for lo, cnt in ranges:
                buf = torch.empty(cnt, dtype=torch.int32, device="cuda")
                ctx.align_range(lo, cnt, buf.data_ptr())
        torch.cuda.synchronize()
        det.enqueue_ms["two contexts on two streams, 6 + 6 ranges"] = two_streams(det, streams, jobs)


def test_one_context_on_two_streams(det, streams, w):
    """what the header promises for sa_ctx_align_range of ONE context on two streams: ranges that run on the tile kernels alone --
    no column beyond 1024 residues, a scoring inside the kernels' limits -- may be in flight on several streams at once (every
    call has counters of its own); here twelve column blocks of the 200 proteins, dealt alternately to two streams"""
    import torch
    ctx = w.ctx
    blocks = column_blocks(N, 12)
    ctx.timing(True)
    for lo, cnt in blocks:
        buf = torch.empty(cnt, dtype=torch.int32, device="cuda")
        ctx.align_range(lo, cnt, buf.data_ptr())
    torch.cuda.synchronize()
    tm = ctx.timing_read()
    ctx.timing(False)
    assert max(w.lens) <= 1024 and tm["kernel"].startswith("sa_k_systolic_pk_bundle<"), f"not a store for the tile kernels alone: {tm}"
    jobs = [(ctx, w.packed["T"], blocks[0::2]), (ctx, w.packed["T"], blocks[1::2])]
    det.enqueue_ms["one context on two streams, 6 + 6 ranges"] = two_streams(det, streams, jobs)
