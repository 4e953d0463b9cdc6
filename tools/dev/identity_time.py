"""tools/dev/identity_time.py [--reps R] [--stores cfg2,large] [--large-pairs P] -- the identity sweep (sa_ctx_identity_range,
csrc/sa_identity.hip) beside its three yardsticks, per method, on config 2's store (10 000 proteins of 80 - 120 residues) and on
40 000 proteins of 96 - 144 residues.  HIP events on a stream of its own, one warm-up call, then the median of R (default 11):

  (a) the same sweep without payloads: sa_k_pair_per_wave (SA_HIP_FORCE_GENERIC, sa_ctx_align_range) over the same packed range.
      The ratio is what the payloads cost.
  (b) the only other way to identities: fill + walk of sa_ctx_alignments on the N x 64 neighbour list
      (sa_hip_last_alignments_breakdown), as DP cells per second against the sweep's.
  (c) the packed alignment of the whole store (sa_hip_last_align_seconds inside sa_hip_neighbors), as context.

The range is the whole triangle; --large-pairs P limits the large store to its last P pairs, column-aligned (the last columns:
the longest row lists), when the whole triangle of 8 x 10^8 pairs takes longer than the run may."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_config, make_protein_set  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps = int(arg("--reps", 11))
which = arg("--stores", "cfg2,large").split(",")
large_pairs = int(arg("--large-pairs", 0))
K = 64
GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}


def timed(call, stream):
    times = []
    for rep in range(1 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        stream.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def run(name, seqs, matrix, cap):
    store = sa.SequenceStore.from_sequences(seqs)
    n = store.num
    start = 0
    if cap and cap < store.pairs:  # the last columns, whole
        j = n - 1
        while j > 1 and store.pairs - j * (j - 1) // 2 < cap:
            j -= 1
        start = j * (j - 1) // 2
    count = store.pairs - start
    cells = store.cells(start, count)
    print(f"\n== {name}: N = {n}, {store.pairs} pairs; the range [{start}, {store.pairs}): {count} pairs, {cells} cells")
    stream = torch.cuda.Stream()
    d_out = torch.empty(count, dtype=torch.int32, device="cuda")
    for method in ("nw", "ga", "sw"):
        scoring = sa.Scoring.from_names(method, matrix, **GAPS[method])
        with sa.Context(store, scoring, 0) as ctx:
            ident = timed(lambda: ctx.identity_range(start, count, pid=d_out.data_ptr(), denom=sa.PID_COLUMNS, stream=stream.cuda_stream), stream)
        os.environ["SA_HIP_FORCE_GENERIC"] = "1"
        try:
            with sa.Context(store, scoring, 0) as ctx:
                plain = timed(lambda: ctx.align_range(start, count, d_out.data_ptr(), stream=stream.cuda_stream), stream)
        finally:
            del os.environ["SA_HIP_FORCE_GENERIC"]
        sa.hip_neighbors(store, scoring, K)  # warm-up: code objects, plans
        index, _ = sa.hip_neighbors(store, scoring, K)
        packed_ms = sa.last_align_seconds() * 1e3
        pairs = np.stack([np.repeat(np.arange(n, dtype=np.int32), K), index.reshape(-1)], axis=1)
        with sa.Context(store, scoring, 0) as ctx:
            ctx.alignments(pairs)
            ctx.alignments(pairs)
            bd = sa.last_alignments_breakdown()
        trace_s = bd["fill_seconds"] + bd["walk_seconds"]
        id_gcups, plain_gcups, trace_gcups = cells / ident[0] / 1e6, cells / plain[0] / 1e6, bd["cells"] / trace_s / 1e9
        print(f"{method}: identity sweep {ident[0]:10.3f} ms ({ident[1]:.3f} .. {ident[2]:.3f}), {id_gcups:7.1f} GCUPS")
        print(f"    (a) pair-per-wave score sweep, same range {plain[0]:10.3f} ms ({plain[1]:.3f} .. {plain[2]:.3f}), {plain_gcups:7.1f} GCUPS: "
              f"identity / score sweep = {ident[0] / plain[0]:.3f}")
        print(f"    (b) traceback of the {len(pairs)} neighbour pairs (K = {K}): fill {bd['fill_seconds'] * 1e3:.3f} ms + walk {bd['walk_seconds'] * 1e3:.3f} ms, "
              f"{bd['cells']} cells, {bd['batches']} batch(es): {trace_gcups:7.1f} GCUPS; identity sweep / traceback, cells per second = {id_gcups / trace_gcups:.2f}")
        print(f"    (c) packed alignment of all {store.pairs} pairs: {packed_ms:10.3f} ms; the identity sweep of the whole triangle would take "
              f"{ident[0] * store.cells() / cells:10.1f} ms at this rate")


print(f"device: {sa.device_name(0)}; one warm-up call, then the median of {reps} (min .. max)")
if "cfg2" in which:
    seqs, cfg = make_config("cfg2")
    run("config 2", seqs, cfg["matrix"], 0)
if "large" in which:
    run("40 000 x 96 - 144 aa", make_protein_set(40000, 96, 144, 5), "blosum62", large_pairs)
