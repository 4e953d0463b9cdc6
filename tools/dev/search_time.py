"""tools/dev/search_time.py [--reps R] -- the search (sa_ctx_search_range + sa_ctx_hits, csrc/sa_search.hip) beside the all-vs-all
alignment of the same database in the same process, everything device-resident and timed with HIP events on one stream: a few
warm-up runs, then the median of R (default 7).

db = config 2's store (10 000 proteins of 80 - 120 residues, NW / BLOSUM62); queries M in {10, 1000, 10 000} from the same
generator under another seed.  Per M:
  - the alignment of the M x N rectangle alone (the bounded range into scratch) as DP cells/s, beside the all-vs-all rate of the
    database (sa_ctx_align_range over its triangle): the same kernels on a rectangle instead of a triangle, not a target figure;
  - search_range as a whole (alignment + the gather sa_k_rect_rows), so the gather's time is the difference;
  - hits at k in {8, 64}: ms, its share of the alignment beside it, the segments per row, and 4 M N bytes / time as a fraction of
    the 8 TB/s HBM roof.
Condition (M = 1000, k = 64): the selection takes no more than 10 % of the alignment beside it."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import CONFIGS, make_config, make_protein_set  # noqa: E402

ROOF = 8e12
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7


def median_ms(stream, fn, warm=2):
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


db_seqs, cfg = make_config("cfg2")
scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
db = sa.SequenceStore.from_sequences(db_seqs)
n = db.num
db_len = sum(len(s) for s in db_seqs)
stream = torch.cuda.Stream()
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 2 warm-ups, median (min .. max)")

d_packed = torch.empty(db.pairs, dtype=torch.int32, device="cuda")
with sa.Context(db, scoring, 0) as ctx:
    all_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, db.pairs, d_packed.data_ptr(), stream=stream.cuda_stream))
    all_rate = db.cells() / (all_ms * 1e-3)
print(f"all-vs-all of the database: N = {n}, {db.pairs} pairs, {db.cells()} cells: {all_ms:.3f} ms ({lo:.3f} .. {hi:.3f}) = {all_rate / 1e12:.3f} T cells/s")
del d_packed

verdict = None
for m in (10, 1000, 10_000):
    query_seqs = make_protein_set(m, CONFIGS["cfg2"]["lo"], CONFIGS["cfg2"]["hi"], 202)
    queries = sa.SequenceStore.from_sequences(query_seqs)
    cells = db_len * sum(len(s) for s in query_seqs)
    with sa.SearchContext(db, queries, scoring, 0) as sx:
        d_scratch = torch.empty(sx.search_scratch_bytes(0, m) // 4, dtype=torch.int32, device="cuda")
        d_rect = torch.empty(m * n, dtype=torch.int32, device="cuda")
        d_out = torch.empty(2 * m * 64, dtype=torch.int32, device="cuda")
        # the alignment alone: the bounded range as search_range runs it (the library's own entry point refuses a search context,
        # so time search_range with kernel timing on and read the alignment kernels' sum)
        sr_ms, lo, hi = median_ms(stream, lambda: sx.search_range(0, m, d_rect.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream))
        sx.timing(True)
        for _ in range(reps):
            sx.search_range(0, m, d_rect.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        t = sx.timing_read()
        sx.timing(False)
        align_ms = t["all_kernels_ms"] / reps
        rate = cells / (align_ms * 1e-3)
        print(f"\nM = {m}: {m * n} pairs, {cells} cells; search_range {sr_ms:.3f} ms ({lo:.3f} .. {hi:.3f}); its alignment kernels {align_ms:.3f} ms "
              f"(mean of {reps}, {t['kernel']}: {t['pairs'] // reps} pairs a run) = {rate / 1e12:.3f} T cells/s = {rate / all_rate:.2f} of the all-vs-all rate; "
              f"gather + launch gaps {sr_ms - align_ms:.3f} ms")
        for k in (8, 64):
            need = sa.hits_scratch_bytes(n, m, k)
            d_part = torch.empty(max(need // 4, 1), dtype=torch.int32, device="cuda")
            ms, lo, hi = median_ms(stream, lambda: sx.hits(d_rect.data_ptr(), m, k, d_out.data_ptr(), d_out.data_ptr() + 4 * m * 64, d_part.data_ptr(),
                                                           stream=stream.cuda_stream))
            segs = need // (8 * m * k)
            print(f"  k = {k:2d}: hits {ms:7.3f} ms ({lo:.3f} .. {hi:.3f}), {max(segs, 1)} segment(s) per row = {m * max(segs, 1)} waves in phase 1  "
                  f"= {100.0 * ms / align_ms:5.2f} % of the alignment;  4 M N bytes / time = {4.0 * m * n / (ms * 1e-3) / ROOF:.4f} of the roof")
            if m == 1000 and k == 64:
                verdict = (ms, align_ms)
ms, align_ms = verdict
print(f"\ncondition (M = 1000, k = 64: selection <= 10 % of the alignment beside it): {ms:.3f} ms of {align_ms:.3f} ms = "
      f"{100.0 * ms / align_ms:.2f} % -> {'MET' if ms <= 0.10 * align_ms else 'MISSED'}")
