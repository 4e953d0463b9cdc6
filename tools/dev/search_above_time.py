"""tools/dev/search_above_time.py [--reps R] [--out FILE] -- the threshold search (sa_ctx_hits_above_offsets + _fill,
csrc/sa_search_above.hip) beside the top-k selection (sa_ctx_hits, k = 64) on the same rectangle and beside the alignment that made
the rectangle, everything device-resident and timed with HIP events on one stream: two warm-up runs, then the median of R (default 7).
Writes what it prints to FILE (default profiles/search_above_time.txt).

Shapes (M, N): (3, 10^6) -- few long rows, the split path at its widest; (1000, 10^5); (20 000, 5 000) -- the rows fill the device,
one segment each.  The sequences are drawn with repetition from 20 000 distinct proteins of 30 - 60 residues (NW / BLOSUM62), so
the rectangle holds real scores.  Per shape the thresholds are NumPy quantiles of a sample of rows copied back (at most 4 10^6
elements): they keep about 0.1 %, 1 % and 10 % of the candidates; the hits E are the device's own count.

Bytes every pass must move, against the 8 TB/s HBM roof: count 4 per element; fill 4 per element + 4 per hit read (the raw score)
+ 12 per hit written (index, value, score) -- 8 written and nothing read per hit without the score."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_protein_set  # noqa: E402

ROOF = 8e12
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "search_above_time.txt")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


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


pool = make_protein_set(20_000, 30, 60, 31)
scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
stream = torch.cuda.Stream()
say(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 2 warm-ups, median (min .. max); roof {ROOF / 1e12:.0f} TB/s")

for m, n in ((3, 1_000_000), (1000, 100_000), (20_000, 5_000)):
    rng = np.random.default_rng(m + n)
    db = sa.SequenceStore.from_sequences([pool[k] for k in rng.integers(0, len(pool), n)])
    queries = sa.SequenceStore.from_sequences([pool[k] for k in rng.integers(0, len(pool), m)])
    elems = m * n
    with sa.SearchContext(db, queries, scoring, 0) as sx:
        d_range = torch.empty(sx.search_scratch_bytes(0, m) // 4, dtype=torch.int32, device="cuda")
        d_rect = torch.empty(elems, dtype=torch.int32, device="cuda")
        align_ms, lo, hi = median_ms(stream, lambda: sx.search_range(0, m, d_rect.data_ptr(), d_range.data_ptr(), stream=stream.cuda_stream))
        del d_range
        need = sa.hits_above_scratch_bytes(n, m)
        segs = (need // 8 - 1) // m
        say(f"\n(M, N) = ({m}, {n}): {elems} candidates; alignment of the rectangle + gather {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f}); "
            f"S = {segs} segment(s) per row = {m * segs} waves")
        # the top-k selection on the same rectangle
        k = 64
        d_part = torch.empty(max(sa.hits_scratch_bytes(n, m, k) // 4, 1), dtype=torch.int32, device="cuda")
        d_topk = torch.empty(2 * m * k, dtype=torch.int32, device="cuda")
        topk_ms, lo, hi = median_ms(stream, lambda: sx.hits(d_rect.data_ptr(), m, k, d_topk.data_ptr(), d_topk.data_ptr() + 4 * m * k, d_part.data_ptr(),
                                                            stream=stream.cuda_stream))
        topk_segs = max(sa.hits_scratch_bytes(n, m, k) // (8 * m * k), 1)
        say(f"  sa_ctx_hits, k = 64 ({topk_segs} segment(s) per row): {topk_ms:.3f} ms ({lo:.3f} .. {hi:.3f}) = "
            f"{4.0 * elems / (topk_ms * 1e-3) / ROOF:.3f} of the roof at 4 bytes per element")
        rows = max(1, min(m, 4_000_000 // n))
        sample = d_rect[:rows * n].cpu().numpy()
        d_offsets = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        d_scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda")
        for keep in (0.001, 0.01, 0.1):
            t = int(np.quantile(sample, 1.0 - keep))
            count = lambda: sx.hits_above_offsets(d_rect.data_ptr(), m, t, d_offsets.data_ptr(), d_scratch.data_ptr(), stream=stream.cuda_stream)  # noqa: E731
            count_ms, clo, chi = median_ms(stream, count)
            e = int(d_offsets[m].item())
            d_out = torch.empty(3 * max(e, 1), dtype=torch.int32, device="cuda")
            p = d_out.data_ptr()
            fill_ms, flo, fhi = median_ms(stream, lambda: sx.hits_above_fill(d_rect.data_ptr(), d_rect.data_ptr(), m, t, d_offsets.data_ptr(),
                                                                             d_scratch.data_ptr(), p, p + 4 * e, p + 8 * e, stream=stream.cuda_stream))
            lean_ms, _, _ = median_ms(stream, lambda: sx.hits_above_fill(d_rect.data_ptr(), 0, m, t, d_offsets.data_ptr(), d_scratch.data_ptr(), p,
                                                                         p + 4 * e, 0, stream=stream.cuda_stream))
            count_roof = 4.0 * elems / (count_ms * 1e-3) / ROOF
            fill_roof = (4.0 * elems + 16.0 * e) / (fill_ms * 1e-3) / ROOF
            lean_roof = (4.0 * elems + 8.0 * e) / (lean_ms * 1e-3) / ROOF
            both = count_ms + fill_ms
            say(f"  T = {t} keeps {100.0 * e / elems:.3f} % (E = {e}): count + scan {count_ms:.3f} ms ({clo:.3f} .. {chi:.3f}) = {count_roof:.3f} of the roof; "
                f"fill {fill_ms:.3f} ms ({flo:.3f} .. {fhi:.3f}) = {fill_roof:.3f} of the roof (without the score {lean_ms:.3f} ms = {lean_roof:.3f}); "
                f"count + scan + fill {both:.3f} ms = {both / topk_ms:.2f} x the top-k selection = {100.0 * both / align_ms:.2f} % of the alignment")
            del d_out
        del d_rect, d_offsets, d_scratch, d_part, d_topk
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
