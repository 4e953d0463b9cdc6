"""What tests/test_gpu_stream_order.py is built from: a detector for work that does not keep the order of its stream.

Every device-resident call of include/seqalign_hip.h is "asynchronous on `stream`".  A test that synchronises the host before
the call and before it reads cannot tell a call that keeps that promise from one that launched on another stream: the values
are right either way.  Here the host never waits.  One case is, all on one side stream S:

  1. the delay        a kernel that spins for a calibrated time and ends by itself (torch.cuda._sleep)
  2. truth over decoy every device input holds a DECOY when the case begins -- valid under the call's contract, with a
                      different expected result -- and a device-to-device copy behind the delay replaces it by the true input
  3. poison           every output is filled with POISON
  4. the call(s)
  5. snapshots        device-to-device copies of the outputs

then S.synchronize(), and the snapshots are compared with the expectation of the true input.  Work that ran early -- on stream 0,
on a private stream without an event edge -- ran during the delay: it read the decoy, and the poison came after it.  Work that ran
late is not in the snapshot.  A call that waits for the device inside is seen by Detector.run too: the stream is idle when the
call returns (`idle`), where a call that only enqueues leaves the delay running.

The delay is calibrated once per session with HIP events; every run measures its own delay with two more events and the host time
of whatever the case put behind it, and check() asserts at least MIN_DELAY_MS and a ratio of ten."""
import time

import numpy as np

POISON32 = -0x5A5A5A5B
POISON64 = -0x5A5A5A5A5A5A5A5B
POISON16 = -0x5A5B
MIN_DELAY_MS = 30.0


def poison_of(dtype) -> int:
    return {4: POISON32, 8: POISON64, 2: POISON16}[np.dtype(dtype).itemsize]


class Run:
    """what one case left: the snapshots as host arrays, the host time of the enqueues behind the delay, the length of the delay as
    HIP events on S measured it, whether S was idle when the last enqueue returned"""

    def __init__(self, snaps, host_ms, delay_ms, idle):
        self.snaps, self.host_ms, self.delay_ms, self.idle = snaps, host_ms, delay_ms, idle


class Detector:
    def __init__(self, torch):
        self.torch = torch
        self.cycles_per_ms = None
        self.measured_ms = None
        self.enqueue_ms = {}  # name of a case -> host milliseconds of its enqueues (printed by the test file)

    # ---- the delay -----------------------------------------------------------------------------------------------------------------
    def _timed_sleep(self, cycles: int) -> float:
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    def calibrate(self) -> None:
        """cycles of torch.cuda._sleep per millisecond, from two timed sleeps (their difference: launch overhead cancels), then
        the length of a MIN_DELAY_MS delay measured as a whole"""
        self._timed_sleep(100_000)  # (loads the kernel)
        a, b = 2_000_000, 20_000_000
        ta, tb = self._timed_sleep(a), self._timed_sleep(b)
        assert tb > ta > 0, f"torch.cuda._sleep does not scale: {a} cycles took {ta} ms, {b} cycles {tb} ms"
        self.cycles_per_ms = (b - a) / (tb - ta)
        self.measured_ms = self._timed_sleep(self.cycles(MIN_DELAY_MS))
        assert self.measured_ms >= MIN_DELAY_MS, f"a delay asked to last {MIN_DELAY_MS} ms lasted {self.measured_ms} ms"

    def cycles(self, ms: float) -> int:
        return int(1.1 * ms * self.cycles_per_ms) + 1  # (a tenth over: the measured length must not fall short of `ms`)

    def sleep(self, ms: float) -> None:
        """the delay on the current stream"""
        self.torch.cuda._sleep(self.cycles(ms))

    # ---- one case ------------------------------------------------------------------------------------------------------------------
    def run(self, stream, inputs, outputs, enqueue, call_stream=None, poison=True, delay_ms=MIN_DELAY_MS, name=None) -> Run:
        """inputs: (buffer, truth, decoy) device tensors of one shape each; outputs: device tensors; enqueue(stream_pointer) issues
        the call(s).  call_stream (the controls): the stream the calls are handed instead of `stream`.  poison=False leaves step 3
        out (the controls: what the misplaced call computed is then still there to be looked at)."""
        torch = self.torch
        for buf, _, decoy in inputs:
            buf.copy_(decoy)
        for o in outputs:  # (so that, without step 3, what a call does not write is known as well)
            o.fill_(poison_of(_np_dtype(torch, o.dtype)))
        snaps = [torch.zeros_like(o) for o in outputs]
        began, ended = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            began.record(stream)
            self.sleep(delay_ms)
            ended.record(stream)
            t0 = time.perf_counter()
            for buf, truth, _ in inputs:
                buf.copy_(truth, non_blocking=True)
            if poison:
                for o in outputs:
                    o.fill_(poison_of(_np_dtype(torch, o.dtype)))
        enqueue((call_stream if call_stream is not None else stream).cuda_stream)
        with torch.cuda.stream(stream):
            for s, o in zip(snaps, outputs):
                s.copy_(o, non_blocking=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        idle = bool(stream.query())
        stream.synchronize()
        torch.cuda.synchronize()  # (the controls' other stream)
        if name is not None:
            self.enqueue_ms[name] = max(host_ms, self.enqueue_ms.get(name, 0.0))
        return Run([s.cpu().numpy() for s in snaps], host_ms, float(began.elapsed_time(ended)), idle)  # (the delay as it was, not as asked for)

    @staticmethod
    def check(run: Run, what: str, unsynced: bool = True) -> None:
        """the delay lasted MIN_DELAY_MS or more and outlasted the enqueues ten times over; and, for a call that promises not to wait
        for the device, S was still busy when the last enqueue returned"""
        assert run.delay_ms >= MIN_DELAY_MS, f"{what}: the delay lasted {run.delay_ms:.2f} ms"
        assert run.delay_ms >= 10.0 * run.host_ms, f"{what}: the enqueues took {run.host_ms:.3f} ms of host time behind a delay of {run.delay_ms:.2f} ms"
        if unsynced:
            assert not run.idle, f"{what}: the stream was idle when the last enqueue returned ({run.host_ms:.3f} ms after the delay was " \
                                 f"enqueued, delay {run.delay_ms:.2f} ms): a call waited for the device"


def _np_dtype(torch, dtype):
    return {torch.int32: np.int32, torch.int64: np.int64, torch.int16: np.int16}[dtype]


def assert_differ(what: str, truth, decoy) -> None:
    """from the reference alone, before the device is asked: every compared output array has another expectation under the decoy"""
    for k, (t, d) in enumerate(zip(truth, decoy)):
        t, d = np.asarray(t), np.asarray(d)
        assert t.shape != d.shape or (t != d).any(), f"{what}: output {k} has the same expectation for truth and decoy"


def padded(want: np.ndarray, size: int) -> np.ndarray:
    """the expectation of an output buffer of `size` elements whose first len(want) the call writes: POISON behind them"""
    out = np.full(size, poison_of(want.dtype), want.dtype)
    out[:want.size] = want.reshape(-1)
    return out
