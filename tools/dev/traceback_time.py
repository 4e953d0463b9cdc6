"""tools/dev/traceback_time.py [--reps R] [--n N] -- alignments of the N x K neighbour pairs (sa_ctx_alignments,
csrc/sa_traceback.hip) beside what precedes them, on config 2's store (10 000 proteins of 80 - 120 residues) at K = 10, per method:

  alignment   device time of the all-vs-all scores inside sa_hip_neighbors (sa_hip_last_align_seconds)
  selection   sa_k_neighbors (sa_hip_last_neighbors_seconds)
  fill, walk  sa_hip_last_alignments_breakdown of sa_ctx_alignments on the pairs (r, neighbour): HIP events around
              sa_k_trace_fill and around sa_k_trace_walk + scan + compaction; one warm-up call, then the median of R (default 5)

and the effective GCUPS of the fill (DP cells of the pairs / fill time) against the nearest existing yardstick, the score-only
sweep it restates: sa_k_pair_per_wave over a packed range of the same store (SA_HIP_FORCE_GENERIC, sa_ctx_align_range, HIP events).
The pairs differ (a packed range against the neighbour pairs) but the lengths are the same store's."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_config  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
n_arg = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else None
K = 10
GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}

seqs, cfg = make_config("cfg2", n_arg)
store = sa.SequenceStore.from_sequences(seqs)
n = store.num
print(f"device: {sa.device_name(0)}; config 2's store: N = {n}, {store.pairs} pairs, {store.cells()} cells; K = {K}: {n * K} pairs to trace back")
print(f"fill / walk: one warm-up call, then the median of {reps} (min .. max)")
for method in ("nw", "ga", "sw"):
    scoring = sa.Scoring.from_names(method, cfg["matrix"], **GAPS[method])
    sa.hip_neighbors(store, scoring, K)  # warm-up: code objects, plans
    index, score = sa.hip_neighbors(store, scoring, K)
    align_ms, select_ms = sa.last_align_seconds() * 1e3, sa.last_neighbors_seconds() * 1e3
    pairs = np.stack([np.repeat(np.arange(n, dtype=np.int32), K), index.reshape(-1)], axis=1)
    fills, walks = [], []
    with sa.Context(store, scoring, 0) as ctx:
        for rep in range(1 + reps):
            alns = ctx.alignments(pairs)
            bd = sa.last_alignments_breakdown()
            if rep:
                fills.append(bd["fill_seconds"] * 1e3)
                walks.append(bd["walk_seconds"] * 1e3)
    assert np.array_equal(alns.records["score"], score.reshape(-1)), "the records' scores are the neighbour scores"
    cells, batches = bd["cells"], bd["batches"]
    fill_ms, walk_ms = statistics.median(fills), statistics.median(walks)
    # the yardstick: the score-only pair-per-wave sweep over a packed range of the same store
    os.environ["SA_HIP_FORCE_GENERIC"] = "1"
    try:
        count = min(store.pairs, 4_000_000)
        start = store.pairs - count
        d_scores = torch.empty(count, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        times = []
        with sa.Context(store, scoring, 0) as ctx:
            for rep in range(1 + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.align_range(start, count, d_scores.data_ptr(), stream=stream.cuda_stream)
                e1.record(stream)
                stream.synchronize()
                if rep:
                    times.append(e0.elapsed_time(e1))
        generic_gcups = store.cells(start, count) / (statistics.median(times) * 1e-3) / 1e9
    finally:
        del os.environ["SA_HIP_FORCE_GENERIC"]
    fill_gcups = cells / (fill_ms * 1e-3) / 1e9
    print(f"\n{method}: alignment {align_ms:.3f} ms, selection {select_ms:.3f} ms; {len(pairs)} pairs, {cells} cells, {batches} batch(es), "
          f"{int(alns.records['columns'].sum())} columns, {len(alns.cigar)} runs")
    print(f"  fill {fill_ms:8.3f} ms ({min(fills):.3f} .. {max(fills):.3f}) = {100 * fill_ms / align_ms:6.2f} % of the alignment;  "
          f"{fill_gcups:7.1f} GCUPS against {generic_gcups:7.1f} GCUPS of the score-only sweep: fill / sweep time per cell = {generic_gcups / fill_gcups:.2f}")
    print(f"  walk {walk_ms:8.3f} ms ({min(walks):.3f} .. {max(walks):.3f}) = {100 * walk_ms / align_ms:6.2f} % of the alignment;  "
          f"{walk_ms * 1e6 / len(pairs):.1f} ns per pair, {walk_ms * 1e6 / max(int(alns.records['columns'].sum()), 1):.2f} ns per column")
