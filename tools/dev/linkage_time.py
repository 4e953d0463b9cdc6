"""tools/dev/linkage_time.py [--reps R] -- the single-linkage tree (sa_ctx_linkage, csrc/sa_linkage.hip) beside the alignment that
feeds it, both device-resident and timed with HIP events on one stream: a few warm-up runs, then the median of R (default 11).

Store: config 2 (10 000 proteins).  Printed: the rounds taken; the whole call; one round and the sort; the alignment and
sa_k_neighbors at k = 8 from the same run (one sweep of the same kind over the same bytes: what a Best sweep is compared with);
4 N^2 bytes / round time as a fraction of the 8 TB/s HBM roof.

The entry point is one call, so a round and the sort are told apart by a second matrix of the same size whose tree takes exactly
one round (all scores equal: the star from 0):  round = (call on the store's matrix - call on the all-equal matrix) / (rounds - 1),
sort + the 256-byte memset = call on the all-equal matrix - round.  A round is the Best sweep plus its four kernels of N threads
(prepare, min, hook, relabel); no figure is a condition."""
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


seqs, cfg = make_config("cfg2")
scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
store = sa.SequenceStore.from_sequences(seqs)
n = store.num
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 3 warm-ups, median (min .. max)")
print(f"roof: {ROOF / 1e12:.0f} TB/s")
d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
d_equal = torch.full((store.pairs,), 7, dtype=torch.int32, device="cuda")
d_out = torch.empty(3 * (n - 1), dtype=torch.int32, device="cuda")
d_scratch = torch.empty(sa.linkage_scratch_bytes(n), dtype=torch.uint8, device="cuda")
d_nb = torch.empty(2 * n * 8, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream()
s = stream.cuda_stream
torch.cuda.synchronize()
with sa.Context(store, scoring, 0) as ctx:
    align_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=s), warm=2)
    print(f"\nconfig 2: N = {n}, {store.pairs} pairs; alignment (sa_ctx_align_range) {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
    rounds = {}
    for name, d in (("store", d_packed), ("all equal", d_equal)):
        with sa.DeflateJob(n, 256, d_packed_ptr=d.data_ptr()) as job:
            job.linkage()
        rounds[name] = sa.last_linkage_rounds()
    p, o, c, w = d_packed.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 8 * (n - 1), d_scratch.data_ptr()
    call_ms, lo, hi = median_ms(stream, lambda: ctx.linkage(p, o, c, w, stream=s))
    print(f"  rounds: {rounds['store']} (bound {max(1, (n - 1).bit_length())}); the all-equal matrix: {rounds['all equal']}")
    print(f"  whole call                    {call_ms:8.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * call_ms / align_ms:5.2f} % of the alignment")
    one_ms, lo, hi = median_ms(stream, lambda: ctx.linkage(d_equal.data_ptr(), o, c, w, stream=s))
    print(f"  whole call, all-equal matrix  {one_ms:8.3f} ms ({lo:.3f} .. {hi:.3f})")
    nb_ms, lo, hi = median_ms(stream, lambda: ctx.neighbors(p, 8, d_nb.data_ptr(), d_nb.data_ptr() + 4 * n * 8, stream=s))
    if rounds["store"] > 1 and rounds["all equal"] == 1:
        round_ms = (call_ms - one_ms) / (rounds["store"] - 1)
        print(f"  one round (by difference)     {round_ms:8.3f} ms;  4 N^2 bytes / time = {4.0 * n * n / (round_ms * 1e-3) / ROOF:.3f} of the roof;  "
              f"{round_ms / nb_ms:.2f} x sa_k_neighbors")
        print(f"  sort + memset (by difference) {one_ms - round_ms:8.3f} ms")
    print(f"  (sa_k_neighbors, k = 8, the same run: {nb_ms:.3f} ms ({lo:.3f} .. {hi:.3f}))")
