"""tools/dev/edges_time.py [--reps R] -- the score graph (sa_ctx_edge_offsets + sa_ctx_edge_fill, csrc/sa_edges.hip) beside the
alignment that feeds it, both device-resident and timed with HIP events on one stream: a few warm-up runs, then the median of R
(default 11).

Stores: config 2 (10 000 proteins) and make_protein_set(40000, 96, 144, 5) (the store of profiles/neighbors_time.txt).
T = the 0.99 quantile of the store's own packed matrix (sa_ctx_select on the device).  Per store: count + scan, fill, and the
three together with their share of the alignment ms of the same store in the same process.  Two comparison figures, neither a
condition: sa_k_neighbors at k = 8 from the same run (one sweep of the same kind), and 8 N^2 bytes / time (the matrix is read
twice) as a fraction of the 8 TB/s HBM roof.

Condition (config 2, T = the 0.99 quantile): count + scan + fill take no more than 10 % of the alignment measured beside them."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_config, make_protein_set  # noqa: E402

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


cfg2_seqs, cfg2 = make_config("cfg2")
stores = [("config 2", cfg2_seqs), ("40000 x 96-144 aa", make_protein_set(40000, 96, 144, 5))]
scoring = sa.Scoring.from_names(cfg2["method"], cfg2["matrix"], **cfg2["gaps"])
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 3 warm-ups, median (min .. max)")
print(f"roof: {ROOF / 1e12:.0f} TB/s")
verdict = None
for name, seqs in stores:
    store = sa.SequenceStore.from_sequences(seqs)
    n = store.num
    d_packed = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    d_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_nb = torch.empty(2 * n * 8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with sa.Context(store, scoring, 0) as ctx:
        align_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, store.pairs, d_packed.data_ptr(), stream=s), warm=2)
        print(f"\n{name}: N = {n}, {store.pairs} pairs; alignment (sa_ctx_align_range) {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
        d_cut = torch.empty(1, dtype=torch.int32, device="cuda")
        d_under = torch.empty(1, dtype=torch.int64, device="cuda")
        d_work = torch.empty(sa.select_scratch_bytes(1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.select(d_packed.data_ptr(), [sa.score_rank(store.pairs, 0.99)], d_cut.data_ptr(), d_under.data_ptr(), d_work.data_ptr(), stream=s)
        stream.synchronize()
        t = int(d_cut.item())
        ctx.edge_offsets(d_packed.data_ptr(), t, d_offsets.data_ptr(), stream=s)
        stream.synchronize()
        e = int(d_offsets[n].item())
        d_out = torch.empty(2 * max(e, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p, o, i, c = d_packed.data_ptr(), d_offsets.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 4 * max(e, 1)
        print(f"  T = {t} (0.99 quantile): E = {e} = {100.0 * e / (n * (n - 1)):.2f} % of the entries, {8 * e / 1e6:.1f} MB of index + score")
        off_ms, lo, hi = median_ms(stream, lambda: ctx.edge_offsets(p, t, o, stream=s))
        print(f"  count + scan        {off_ms:7.3f} ms ({lo:.3f} .. {hi:.3f})")
        fill_ms, lo, hi = median_ms(stream, lambda: ctx.edge_fill(p, t, o, i, c, stream=s))
        print(f"  fill                {fill_ms:7.3f} ms ({lo:.3f} .. {hi:.3f})")
        ms, lo, hi = median_ms(stream, lambda: (ctx.edge_offsets(p, t, o, stream=s), ctx.edge_fill(p, t, o, i, c, stream=s)))
        frac = 8.0 * n * n / (ms * 1e-3) / ROOF
        print(f"  count + scan + fill {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * ms / align_ms:5.2f} % of the alignment;  "
              f"8 N^2 bytes / time = {frac:.3f} of the roof")
        nb_ms, lo, hi = median_ms(stream, lambda: ctx.neighbors(p, 8, d_nb.data_ptr(), d_nb.data_ptr() + 4 * n * 8, stream=s))
        print(f"  (sa_k_neighbors, k = 8, the same run: {nb_ms:.3f} ms ({lo:.3f} .. {hi:.3f}))")
        if name == "config 2":
            verdict = (ms, align_ms)
ms, align_ms = verdict
print(f"\ncondition (config 2, T = the 0.99 quantile: count + scan + fill <= 10 % of the alignment beside them): {ms:.3f} ms of "
      f"{align_ms:.3f} ms = {100.0 * ms / align_ms:.2f} % -> {'MET' if ms <= 0.10 * align_ms else 'MISSED'}")
