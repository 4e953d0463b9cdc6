"""GPU (-m gpu): the list form of the fit sweep keeps the order of its stream (include/seqalign_hip.h: sa_ctx_fit_pairs,
"asynchronous on `stream`", the index arrays "read by the kernel in stream order").  The detector is tests/stream_order.py, used as
tests/test_gpu_strands_stream_order.py uses it: behind a calibrated delay on a side stream the true index arrays are copied over
decoys, the outputs are poisoned, the calls are issued and the outputs copied into snapshots, and the host waits for nothing in
between.  Truth and decoy are two lists of (query, database sequence) over one store; the expectation of both comes from
tests/fit_ref.py; every element of every output buffer is compared, the room behind a result included.

1. the call once, all six outputs
2. queued twice on one context behind one delay, each call into buffers of its own, the second with another denominator
Both with nothing synchronised: the stream is still busy when the last enqueue returns.

The side stream is this file's own, made with hipStreamCreateWithFlags and destroyed when the file is done: torch.cuda.Stream()
hands out the streams of a pool in turn, so taking one here would move every later test of the process -- the controls of
tests/test_gpu_stream_order.py among them, which need two streams that the runtime does not put on one hardware queue -- to other
streams than it runs on without this file."""
import ctypes
import types

import numpy as np
import pytest

from tests import fit_ref
from tests.stream_order import assert_differ
from tests.synth import make_protein_set
from tests.test_gpu_fit import LONGER, OUTPUTS, SHORTER, planted
from tests.test_gpu_stream_order import Case, det, execute, keeps_order, same  # noqa: F401  (det: a fixture)

pytestmark = pytest.mark.gpu

N_DB, M_Q, ITEMS, ROOM = 60, 7, 200, 264


def hip_runtime():
    """the HIP runtime this process has loaded (one per process: sequencealigner_amd.binding sees to that)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    return ctypes.CDLL(next((p for p in paths if "/torch/" in p), paths[0]))  # (torch's own copy is the one its streams live in)


@pytest.fixture(scope="module")
def streams(det, sa):  # noqa: F811
    """one side stream, used once for everything a case enqueues as tests/test_gpu_stream_order.py warms its own"""
    import torch
    torch.cuda.synchronize()  # (the runtime is up)
    hip = hip_runtime()
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    handle = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(handle), 1) == 0 and handle.value  # (1: hipStreamNonBlocking, as the pool's streams are)
    s = torch.cuda.ExternalStream(handle.value)
    with torch.cuda.stream(s):
        det.sleep(0.1)
        a = torch.zeros(64, dtype=torch.int32, device="cuda")
        a.fill_(1)
        torch.empty_like(a).copy_(a, non_blocking=True)
    s.synchronize()
    yield (s,)
    torch.cuda.synchronize()
    assert hip.hipStreamDestroy(handle) == 0


@pytest.fixture(scope="module")
def ft(sa):
    db = make_protein_set(N_DB, 20, 66, 601)
    queries = make_protein_set(M_Q, 8, 25, 602)
    short, long = next(s for s in db if 30 <= len(s) < 40), next(s for s in db if len(s) >= 60)
    queries[2] = planted(short, 7, 20, 3)
    queries[4] = planted(long, 30, 25, 4)
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    ref = [[fit_ref.fit_pair(scoring, d, q) for d in db] for q in queries]
    rng = np.random.default_rng(603)
    lists = {k: (rng.integers(0, M_Q, ITEMS).astype(np.int32), rng.integers(0, N_DB, ITEMS).astype(np.int32)) for k in "TD"}

    def want(k, denom):
        q, d = lists[k]
        cols = {name: np.array([ref[a][b][name] for a, b in zip(q, d)], np.int32) for name in OUTPUTS[:5]}
        cols["pid"] = np.array([fit_ref.pid(ref[a][b]["identities"], ref[a][b]["columns"], len(db[b]), len(queries[a]), denom) for a, b in zip(q, d)],
                               np.int32)
        return [cols[name] for name in OUTPUTS]

    ctx = sa.SearchContext(sa.SequenceStore.from_sequences(db), sa.SequenceStore.from_sequences(queries), scoring, 0)
    yield types.SimpleNamespace(ctx=ctx, lists=lists, want=want)
    ctx.close()


def pointers(o, first=0):
    return dict(zip(OUTPUTS, o[first:first + 6]))


def test_fit_pairs_keeps_stream_order(det, streams, ft):  # noqa: F811
    ctx = ft.ctx
    case = Case("fit_pairs", [(ft.lists["T"][0], ft.lists["D"][0]), (ft.lists["T"][1], ft.lists["D"][1])], [(np.int32, ROOM)] * 6,
                {k: ft.want(k, SHORTER) for k in "TD"},
                lambda i, o, x, s: ctx.fit_pairs(i[0], i[1], ITEMS, denom=SHORTER, stream=s, **pointers(o)), warm=True)
    keeps_order(det, streams[0], case)


def test_queued_twice_on_one_context(det, streams, ft):  # noqa: F811
    """two list sweeps of one context behind one delay, the second over the reversed list and under another denominator: the second
    call's launch parameters must not reach the first's kernel, and both share the context's boundary scratch in stream order"""
    ctx = ft.ctx
    rev = {k: (ft.lists[k][0][::-1].copy(), ft.lists[k][1][::-1].copy()) for k in "TD"}
    want = {k: ft.want(k, SHORTER) + [a[::-1].copy() for a in ft.want(k, LONGER)] for k in "TD"}
    assert_differ("queued twice", want["T"], want["D"])
    assert (want["T"][5] != want["T"][11][::-1]).any()  # the two denominators tell the calls apart

    def enqueue(i, o, x, s):
        ctx.fit_pairs(i[0], i[1], ITEMS, denom=SHORTER, stream=s, **pointers(o))
        ctx.fit_pairs(i[2], i[3], ITEMS, denom=LONGER, stream=s, **pointers(o, 6))
    inputs = [(ft.lists["T"][0], ft.lists["D"][0]), (ft.lists["T"][1], ft.lists["D"][1]), (rev["T"][0], rev["D"][0]), (rev["T"][1], rev["D"][1])]
    case = Case("fit_pairs x 2", inputs, [(np.int32, ROOM)] * 12, want, enqueue, warm=True)
    for name in (None, case.name):
        run = execute(det, streams[0], case, name=name)
        same(case.name, run.snaps, want["T"])
        det.check(run, case.name)
