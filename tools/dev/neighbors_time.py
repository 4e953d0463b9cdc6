"""tools/dev/neighbors_time.py [--reps R] -- the nearest-neighbour selection (sa_ctx_neighbors, csrc/sa_neighbors.hip)
beside the alignment that feeds it, both device-resident and timed with HIP events on one stream: a few warm-up runs, then the
median of R (default 11).

Stores: config 2 (10 000 proteins) and make_protein_set(40000, 96, 144, 5) (the store of profiles/z79_deflate_time_n40000.txt);
k in {8, 32, 64}.  Per line: selection ms, its share of the alignment ms of the same store in the same process, and
4 N^2 bytes / time as a fraction of the 8 TB/s HBM roof -- beside 0.55, what sa_k_tiles_raw (the one comparable kernel on record:
the same packed triangle read as 64 x 64 blocks turned in LDS) reaches.

Condition (config 2, k = 64): the selection takes no more than 10 % of the alignment measured beside it."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_config, make_protein_set  # noqa: E402

ROOF = 8e12
TILES_RAW = 0.55
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


cfg2_seqs, cfg2 = make_config("cfg2")
stores = [("config 2", cfg2_seqs), ("40000 x 96-144 aa", make_protein_set(40000, 96, 144, 5))]
scoring = sa.Scoring.from_names(cfg2["method"], cfg2["matrix"], **cfg2["gaps"])
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 3 warm-ups, median (min .. max)")
print(f"roof: {ROOF / 1e12:.0f} TB/s; sa_k_tiles_raw on record: {TILES_RAW:.2f} of it")
verdict = None
for name, seqs in stores:
    store = sa.SequenceStore.from_sequences(seqs)
    n = store.num
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_out = torch.empty(2 * n * 64, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    with sa.Context(store, scoring, 0) as ctx:
        align_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=stream.cuda_stream), warm=2)
        print(f"\n{name}: N = {n}, {store.pairs} pairs; alignment (sa_ctx_align_range) {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
        for k in (8, 32, 64):
            ms, lo, hi = median_ms(stream, lambda: ctx.neighbors(d_packed.data_ptr(), k, d_out.data_ptr(), d_out.data_ptr() + 4 * n * 64,
                                                                  stream=stream.cuda_stream))
            frac = 4.0 * n * n / (ms * 1e-3) / ROOF
            print(f"  k = {k:2d}: selection {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * ms / align_ms:5.2f} % of the alignment;  "
                  f"4 N^2 bytes / time = {frac:.3f} of the roof (sa_k_tiles_raw: {TILES_RAW:.2f})")
            if name == "config 2" and k == 64:
                verdict = (ms, align_ms)
ms, align_ms = verdict
print(f"\ncondition (config 2, k = 64: selection <= 10 % of the alignment beside it): {ms:.3f} ms of {align_ms:.3f} ms = "
      f"{100.0 * ms / align_ms:.2f} % -> {'MET' if ms <= 0.10 * align_ms else 'MISSED'}")
