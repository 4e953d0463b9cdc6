"""tools/dev/select_time.py [--reps R] -- the order statistics of the score distribution (sa_ctx_select, csrc/sa_select.hip)
beside the alignment that feeds them, both device-resident and timed with HIP events on one stream: a few warm-up runs, then the
median of R (default 11).

Store: config 2 (10 000 proteins, P = 49 995 000 pairs).  One call for m = 1 (the 0.99 quantile) and one for m = 16 (the
fractions k / 15), each the start kernel and four count + narrow rounds; with their share of the alignment ms of the same store
in the same process, and the bytes the four rounds read (4 P bytes each) / time as a fraction of the 8 TB/s HBM roof.  The answers
are checked against torch.sort of the same device matrix before anything is timed.

Condition (config 2): the select of one rank takes no more than 10 % of the alignment measured beside it."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_config  # noqa: E402

ROOF = 8e12
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 11


def median_ms(stream, fn, warm=3):
    times = []
    for rep in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        if rep >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


seqs, cfg2 = make_config("cfg2")
scoring = sa.Scoring.from_names(cfg2["method"], cfg2["matrix"], **cfg2["gaps"])
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 3 warm-ups, median (min .. max)")
print(f"roof: {ROOF / 1e12:.0f} TB/s")
store = sa.SequenceStore.from_sequences(seqs)
n, pairs = store.num, store.pairs
d_packed = torch.empty(pairs, dtype=torch.int32, device="cuda")
d_value = torch.empty(16, dtype=torch.int32, device="cuda")
d_below = torch.empty(16, dtype=torch.int64, device="cuda")
d_scratch = torch.empty(sa.select_scratch_bytes(16), dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
s = stream.cuda_stream
verdict = None
with sa.Context(store, scoring, 0) as ctx:
    align_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, pairs, d_packed.data_ptr(), stream=s), warm=2)
    print(f"\nconfig 2: N = {n}, P = {pairs} pairs ({4 * pairs / 1e6:.0f} MB); alignment (sa_ctx_align_range) {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
    ordered = torch.sort(d_packed).values
    for m, fractions in ((1, [0.99]), (16, [k / 15 for k in range(16)])):
        ranks = [sa.score_rank(pairs, q) for q in fractions]
        p, v, b, w = d_packed.data_ptr(), d_value.data_ptr(), d_below.data_ptr(), d_scratch.data_ptr()
        ctx.select(p, ranks, v, b, w, stream=s)
        stream.synchronize()
        want = ordered[torch.tensor(ranks, device="cuda")]
        want_below = torch.searchsorted(ordered, want)
        assert torch.equal(d_value[:m], want) and torch.equal(d_below[:m], want_below), "select differs from torch.sort"
        ms, lo, hi = median_ms(stream, lambda: ctx.select(p, ranks, v, b, w, stream=s))
        frac = 4.0 * pairs * 4 / (ms * 1e-3) / ROOF
        print(f"  select, m = {m:2d}      {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * ms / align_ms:5.2f} % of the alignment;  "
              f"4 P bytes x 4 rounds / time = {frac:.3f} of the roof")
        if m == 1:
            print(f"    (T = {int(d_value[0].item())} at the 0.99 quantile, rank {ranks[0]}: {pairs - int(d_below[0].item())} pairs at or above it)")
            verdict = (ms, align_ms)
ms, align_ms = verdict
print(f"\ncondition (config 2, one rank: select <= 10 % of the alignment beside it): {ms:.3f} ms of "
      f"{align_ms:.3f} ms = {100.0 * ms / align_ms:.2f} % -> {'MET' if ms <= 0.10 * align_ms else 'MISSED'}")
