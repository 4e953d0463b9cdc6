"""tools/dev/agglo_time.py [--reps R] -- complete and average linkage (sa_ctx_agglomerate, csrc/sa_agglo.hip) beside the alignment
that feeds them and the single-linkage tree of the same matrix, all device-resident and timed with HIP events on one stream: a
warm-up run, then the median of R (default 5).

Store: config 2 (10 000 proteins).  Printed per method: the whole call (expand + first scan + N - 1 steps), the call divided by
the steps, the row rescans, and the same on an all-equal matrix (no rescan: what 2 (N - 1) launches and row a cost when nothing
else happens).  The entry point is one call, so expand + first scan are not told apart from the steps here; the step is two small
kernels, and the empty-launch figure printed last (a one-element torch fill on the same stream) says what two launches cost by
themselves.  On the host: scipy.cluster.hierarchy.linkage on the 2 000-sequence prefix, what users do today.  No figure is a
condition."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_config  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5


def median_ms(stream, fn, warm=1):
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


seqs, cfg = make_config("cfg2")
scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
store = sa.SequenceStore.from_sequences(seqs)
n = store.num
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after a warm-up, median (min .. max)")
d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
d_equal = torch.full((store.pairs,), 7, dtype=torch.int32, device="cuda")
d_out = torch.empty(3 * (n - 1), dtype=torch.int32, device="cuda")
d_scratch = torch.empty(sa.agglo_scratch_bytes(n, "average"), dtype=torch.uint8, device="cuda")
d_one = torch.zeros(1, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream()
s = stream.cuda_stream
torch.cuda.synchronize()
with sa.Context(store, scoring, 0) as ctx:
    align_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=s))
    print(f"\nconfig 2: N = {n}, {store.pairs} pairs; alignment (sa_ctx_align_range) {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
    p, o, c, w = d_packed.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 8 * (n - 1), d_scratch.data_ptr()
    single_ms, lo, hi = median_ms(stream, lambda: ctx.linkage(p, o, c, w, stream=s))  # (its scratch is far smaller)
    print(f"  single linkage (sa_ctx_linkage) {single_ms:9.3f} ms ({lo:.3f} .. {hi:.3f})")
    for method in ("complete", "average"):
        rescans = {}
        for name, d in (("store", d_packed), ("all equal", d_equal)):
            with sa.DeflateJob(n, 256, d_packed_ptr=d.data_ptr()) as job:
                job.agglomerate(method)
            rescans[name] = sa.last_agglomerate_rescans()
        call_ms, lo, hi = median_ms(stream, lambda: ctx.agglomerate(p, method, o, c, w, stream=s))
        print(f"  {method} linkage: scratch {sa.agglo_scratch_bytes(n, method) / 2**20:.0f} MiB")
        print(f"    whole call                    {call_ms:9.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * call_ms / align_ms:6.2f} % of the alignment, "
              f"{call_ms / single_ms:.1f} x single linkage")
        print(f"    call / (N - 1) steps          {1e3 * call_ms / (n - 1):9.3f} us; {rescans['store']} row rescans, {rescans['store'] / (n - 1):.2f} per step")
        equal_ms, lo, hi = median_ms(stream, lambda: ctx.agglomerate(d_equal.data_ptr(), method, o, c, w, stream=s))
        print(f"    all-equal matrix              {equal_ms:9.3f} ms ({lo:.3f} .. {hi:.3f}); / (N - 1) = {1e3 * equal_ms / (n - 1):.3f} us; "
              f"{rescans['all equal']} row rescans")
with torch.cuda.stream(stream):
    launch_ms, lo, hi = median_ms(stream, lambda: [d_one.fill_(1) for _ in range(2000)])
print(f"  two empty-handed launches (2 000 one-element fills / 1 000): {launch_ms:.3f} us ({lo:.3f} .. {hi:.3f})")

m = 2000
try:
    from scipy.cluster import hierarchy
    tri = d_packed[:m * (m - 1) // 2].cpu().numpy()
    print(f"\nhost, the {m}-sequence prefix ({tri.size} pairs): scipy.cluster.hierarchy.linkage on a float64 condensed copy")
    full = np.zeros((m, m), np.float64)  # (scipy's condensed order is by rows, the packed triangle is by columns)
    for col in range(1, m):
        full[:col, col] = full[col, :col] = -tri[col * (col - 1) // 2: col * (col - 1) // 2 + col].astype(np.float64)
    condensed = full[np.triu_indices(m, 1)]
    for method in ("complete", "average"):
        t0 = time.perf_counter()
        hierarchy.linkage(condensed, method)
        print(f"  {method:9s} {1e3 * (time.perf_counter() - t0):9.3f} ms (one run)")
    with sa.DeflateJob(m, 256, d_packed_ptr=d_packed.data_ptr()) as job:
        for method in ("complete", "average"):
            job.agglomerate(method)
            print(f"  device, the same prefix, {method:9s} {1e3 * sa.last_agglomerate_seconds():9.3f} ms")
except ImportError:
    print("\nscipy is not installed: no host comparison")
