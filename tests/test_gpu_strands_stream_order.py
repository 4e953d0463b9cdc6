"""GPU (-m gpu): the three device-resident calls of the two-strand search keep the order of their stream (include/seqalign_hip.h:
sa_ctx_strand_fold, sa_ctx_hits_strand, sa_ctx_hits_above_strand: "asynchronous on `stream`", "never synchronise with the host").
The detector is tests/stream_order.py, used as tests/test_gpu_stream_order.py uses it: behind a calibrated delay on a side stream
the true inputs are copied over decoys, the outputs are poisoned, the calls are issued and the outputs copied into snapshots, and
the host waits for nothing in between.  Truth: the SW rectangles of both strands, decoy: the NW rectangles, both from the oracle
(tests/strands_cases.py); every element of every output buffer is compared, the room behind a result included.

The detector's buffers are int32 / int64.  The strands are bytes: they are written into an int32 buffer and compared as the int32
words those bytes make, the poison's bytes behind them.

1. each call once, truth over decoy; the fold with and without the raw scores carried
2. queued twice on one context behind one delay: two folds and their strand takes, each into buffers of its own
3. on two streams: one context, a fold and a strand take on each, enqueued alternately
All of it with nothing synchronised: the stream is still busy when the last enqueue returns."""
import time
import types

import numpy as np
import pytest

from tests import tables
from tests.strands_cases import Folded, dna_database, dna_queries, folded_case
from tests.stream_order import MIN_DELAY_MS, assert_differ, poison_of
from tests.test_gpu_normalize import MIN, normalized
from tests.test_gpu_stream_order import DELAY_MS, Case, det, execute, keeps_order, same, streams  # noqa: F401  (det, streams: fixtures)

pytestmark = pytest.mark.gpu

N_DB, M_Q, K_HITS = 130, 7, 5
WORDS = (N_DB + 63) // 64


def as_words(strand_bytes: np.ndarray, room: int) -> np.ndarray:
    """uint8 results as the int32 words of a poisoned buffer of `room` int32 that holds them"""
    buf = np.full(4 * room, 0xA5, np.uint8)  # (the bytes of POISON32)
    assert poison_of(np.int32) & 0xFF == 0xA5 and strand_bytes.size <= buf.size
    buf[:strand_bytes.size] = strand_bytes.reshape(-1)
    return buf.view(np.int32)


@pytest.fixture(scope="module")
def st(sa, oracle):
    db_seqs = dna_database(N_DB, seed=501)
    query_seqs = dna_queries(db_seqs, M_Q, seed=502)
    scoring = {"T": sa.Scoring.from_names("sw", "nuc44", **tables.GAPS["sw"]), "D": sa.Scoring.from_names("nw", "nuc44", **tables.GAPS["nw"])}
    exp = {k: folded_case(sa, oracle, db_seqs, query_seqs, scoring[k]) for k in "TD"}
    den_d, den_q = 50 + np.arange(N_DB) % 37, 40 + np.arange(M_Q) % 11  # values that are not the scores: NumPy's own division
    vexp = {k: Folded(exp[k].fwd, exp[k].rev, normalized(exp[k].fwd, den_d[None, :], den_q[:, None], MIN),
                      normalized(exp[k].rev, den_d[None, :], den_q[:, None], MIN)) for k in "TD"}
    ctx = sa.SearchContext(sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs), scoring["T"], 0, strands=True)
    yield types.SimpleNamespace(exp=exp, vexp=vexp, ctx=ctx)
    ctx.close()


def strands_case(name, st):
    ctx, i32, i64 = st.ctx, np.int32, np.int64
    both = lambda f: {k: f(k) for k in "TD"}  # noqa: E731
    e, v = st.exp, st.vexp
    rects = [(e["T"].fwd, e["D"].fwd), (e["T"].rev, e["D"].rev)]
    room = M_Q * N_DB
    if name == "strand_fold":
        return Case(name, rects, [(i32, room), (i64, M_Q * WORDS)], both(lambda k: [e[k].best.reshape(-1), e[k].bits().view(i64).reshape(-1)]),
                    lambda i, o, x, s: ctx.strand_fold(i[0], i[1], M_Q, o[0], o[1], stream=s), warm=True)
    if name == "strand_fold with scores":
        values = [(v["T"].vfwd, v["D"].vfwd), (v["T"].vrev, v["D"].vrev)]
        return Case(name, values + rects, [(i32, room), (i32, room), (i64, M_Q * WORDS)],
                    both(lambda k: [v[k].vbest.reshape(-1), v[k].best.reshape(-1), v[k].bits().view(i64).reshape(-1)]),
                    lambda i, o, x, s: ctx.strand_fold(i[0], i[1], M_Q, o[0], o[2], d_sfwd_ptr=i[2], d_srev_ptr=i[3], d_sbest_ptr=o[1], stream=s), warm=True)
    if name == "hits_strand":  # the bitmap and the indices are device inputs: the hits of each expectation
        hits = both(lambda k: e[k].hits(K_HITS))
        words = (M_Q * K_HITS + 3) // 4 + 2
        return Case(name, [(e["T"].bits().view(i64), e["D"].bits().view(i64)), (hits["T"][0], hits["D"][0])], [(i32, words)],
                    both(lambda k: [as_words(hits[k][3], words)]), lambda i, o, x, s: ctx.hits_strand(i[0], M_Q, K_HITS, i[1], o[0], stream=s), warm=True)
    if name == "hits_above_strand":  # offsets and indices of each expectation's CSR at the truth's third quartile, the indices in nq * N of room
        t = int(np.sort(e["T"].best.reshape(-1))[room * 3 // 4])
        csr = both(lambda k: e[k].above(t))
        index = both(lambda k: np.concatenate([csr[k][1], np.zeros(room - csr[k][1].size, np.int32)]))
        words = (room + 3) // 4
        return Case(name, [(e["T"].bits().view(i64), e["D"].bits().view(i64)), (csr["T"][0], csr["D"][0]), (index["T"], index["D"])], [(i32, words)],
                    both(lambda k: [as_words(csr[k][4], words)]), lambda i, o, x, s: ctx.hits_above_strand(i[0], M_Q, i[1], i[2], o[0], stream=s), warm=True)
    raise KeyError(name)


CALLS = ["strand_fold", "strand_fold with scores", "hits_strand", "hits_above_strand"]


# ---- 1. each call once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CALLS)
def test_strands_call_keeps_stream_order(name, det, streams, st):  # noqa: F811
    keeps_order(det, streams[0], strands_case(name, st))


# ---- 2. queued twice on one context ------------------------------------------------------------------------------------------------------
def test_queued_twice_on_one_context(det, streams, st):  # noqa: F811
    """fold by score and fold by value of one context behind one delay, each followed by the strand take of its own hits: the second
    call's launch parameters must not reach the first's kernels"""
    ctx, e, v = st.ctx, st.exp, st.vexp
    room, words = M_Q * N_DB, (M_Q * K_HITS + 3) // 4 + 2
    hits = {k: (e[k].hits(K_HITS), v[k].hits(K_HITS)) for k in "TD"}
    want = {k: [e[k].best.reshape(-1), e[k].bits().view(np.int64).reshape(-1), as_words(hits[k][0][3], words),
                v[k].vbest.reshape(-1), v[k].best.reshape(-1), v[k].bits().view(np.int64).reshape(-1), as_words(hits[k][1][3], words)] for k in "TD"}
    assert_differ("queued twice", want["T"], want["D"])

    def enqueue(i, o, x, s):
        ctx.strand_fold(i[0], i[1], M_Q, o[0], o[1], stream=s)
        ctx.strand_fold(i[2], i[3], M_Q, o[3], o[5], d_sfwd_ptr=i[0], d_srev_ptr=i[1], d_sbest_ptr=o[4], stream=s)
        ctx.hits_strand(o[1], M_Q, K_HITS, i[4], o[2], stream=s)
        ctx.hits_strand(o[5], M_Q, K_HITS, i[5], o[6], stream=s)
    inputs = [(e["T"].fwd, e["D"].fwd), (e["T"].rev, e["D"].rev), (v["T"].vfwd, v["D"].vfwd), (v["T"].vrev, v["D"].vrev),
              (hits["T"][0][0], hits["D"][0][0]), (hits["T"][1][0], hits["D"][1][0])]
    outputs = [(np.int32, room), (np.int64, M_Q * WORDS), (np.int32, words), (np.int32, room), (np.int32, room), (np.int64, M_Q * WORDS), (np.int32, words)]
    case = Case("strand_fold x 2 -> hits_strand x 2", inputs, outputs, want, enqueue, warm=True)
    for name in (None, case.name):
        run = execute(det, streams[0], case, name=name)
        same(case.name, run.snaps, want["T"])
        det.check(run, case.name)


# ---- 3. on two streams ---------------------------------------------------------------------------------------------------------------------
def test_one_context_on_two_streams(det, streams, st):  # noqa: F811
    """the calls keep no state in the context: a fold and a strand take on each of two streams, enqueued alternately behind a delay
    on each, the inputs of each stream copied over decoys behind its delay"""
    torch = det.torch
    ctx, e, v = st.ctx, st.exp, st.vexp
    words = (M_Q * K_HITS + 3) // 4 + 2
    jobs = []
    for exp in (e, v):  # stream 0: by score; stream 1: by value
        hits = {k: exp[k].hits(K_HITS) for k in "TD"}
        ins = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (exp[k].vfwd, exp[k].vrev, hits[k][0])] for k in "TD"]
        bufs = [torch.empty_like(t) for t in ins[0]]
        outs = [torch.empty(M_Q * N_DB, dtype=torch.int32, device="cuda"), torch.empty(M_Q * WORDS, dtype=torch.int64, device="cuda"),
                torch.empty(words, dtype=torch.int32, device="cuda")]
        want = [exp["T"].vbest.reshape(-1), exp["T"].bits().view(np.int64).reshape(-1), as_words(hits["T"][3], words)]
        assert_differ("two streams", want, [exp["D"].vbest.reshape(-1), exp["D"].bits().view(np.int64).reshape(-1), as_words(hits["D"][3], words)])
        jobs.append(types.SimpleNamespace(truth=ins[0], decoy=ins[1], bufs=bufs, outs=outs, snaps=[torch.zeros_like(o) for o in outs], want=want))
    for job in jobs:
        for b, d in zip(job.bufs, job.decoy):
            b.copy_(d)
    torch.cuda.synchronize()
    marks = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in streams]
    for s, (began, ended) in zip(streams, marks):
        with torch.cuda.stream(s):
            began.record(s)
            det.sleep(DELAY_MS)
            ended.record(s)
    t0 = time.perf_counter()
    for s, job in zip(streams, jobs):
        with torch.cuda.stream(s):
            for b, t in zip(job.bufs, job.truth):
                b.copy_(t, non_blocking=True)
            for o in job.outs:
                o.fill_(poison_of(np.int32 if o.dtype == torch.int32 else np.int64))
    for s, job in zip(streams, jobs):
        ctx.strand_fold(job.bufs[0].data_ptr(), job.bufs[1].data_ptr(), M_Q, job.outs[0].data_ptr(), job.outs[1].data_ptr(), stream=s.cuda_stream)
    for s, job in zip(streams, jobs):
        ctx.hits_strand(job.outs[1].data_ptr(), M_Q, K_HITS, job.bufs[2].data_ptr(), job.outs[2].data_ptr(), stream=s.cuda_stream)
    for s, job in zip(streams, jobs):
        with torch.cuda.stream(s):
            for snap, o in zip(job.snaps, job.outs):
                snap.copy_(o, non_blocking=True)
    host_ms = (time.perf_counter() - t0) * 1e3
    idle = [bool(s.query()) for s in streams]
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    lasted = min(a.elapsed_time(b) for a, b in marks)
    assert lasted >= MIN_DELAY_MS and lasted >= 10 * host_ms, f"the enqueues took {host_ms:.3f} ms behind delays of {lasted:.2f} ms"
    assert not any(idle), f"a stream was idle when the last enqueue returned: {idle}"
    for k, job in enumerate(jobs):
        same(f"two streams, stream {k}", [snap.cpu().numpy() for snap in job.snaps], job.want)
    det.enqueue_ms["strands: one context on two streams, fold + strand take each"] = host_ms
