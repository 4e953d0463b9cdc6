"""tools/dev/search_quantity_time.py [--reps R] [--out FILE] -- what ranking the hits of a search by a value costs
(csrc/sa_search_quantity.hip, the rectangle form of sa_k_identity), beside the alignment of the same rectangle in the same process,
everything device-resident and timed with HIP events on one stream: two warm-up runs, then the median of R (default 7).  The report
goes to FILE (default profiles/search_quantity_time.txt) and to stdout.

db = config 2's store (10 000 proteins of 80 - 120 residues, NW / BLOSUM62); queries M in {10, 1000} from the same generator under
another seed.  Per M:
  normalised  sa_ctx_search_range and its alignment kernels; then sa_ctx_denominators (self-scores of the N + M sequences),
              sa_ctx_normalize_rect (MIN, out of place) and sa_ctx_hits_take (k = 64): each in ms, their sum as a share of the alignment
              beside it, and the sweep's 8 M N bytes / time as a fraction of the 8 TB/s HBM roof.
              Condition (M = 1000), the project's own for a quantity: no more than 10 % of the alignment beside it.
  identity    sa_ctx_identity_rect (score and pid together) in DP cells/s, beside sa_ctx_identity_range over a triangle range of the
              same number of pairs of the concatenated store; the two share a body, so the rectangle form may not be slower per cell
              than the triangle form by more than the run-to-run spread printed here ((max - min) / median, the larger of the two).
              The sweeps take turns run by run.  Two triangle ranges are timed and judged: [0, M N), the first columns of the database -- its rows are the first
              sqrt(2 M N) sequences only -- and [tri(N), tri(N) + M N), the query columns themselves with all N database sequences
              (and a few queries) as rows: the pairs of the rectangle but for M (M - 1) / 2 of them, the same row working set.
              Its ratio to the packed alignment of the same rectangle is reported and not judged: that is the known price of the
              payloads."""
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import CONFIGS, make_config, make_protein_set  # noqa: E402

ROOF = 8e12
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "search_quantity_time.txt")
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


def median_ms_in_turns(stream, fns, warm=2):
    """the same for several calls that take turns: run 1 of each, run 2 of each, ..."""
    times = [[] for _ in fns]
    for rep in range(warm + reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            if rep >= warm:
                times[k].append(e0.elapsed_time(e1))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def spread(t):
    return (t[2] - t[1]) / t[0]


db_seqs, cfg = make_config("cfg2")
scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
db = sa.SequenceStore.from_sequences(db_seqs)
n = db.num
db_len = sum(len(s) for s in db_seqs)
stream = torch.cuda.Stream()
s = stream.cuda_stream
say(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 2 warm-ups, median (min .. max)")
say(f"database: config 2, N = {n} proteins, {db_len} residues, {cfg['method']} / {cfg['matrix']}")

verdicts = []
for m in (10, 1000):
    query_seqs = make_protein_set(m, CONFIGS["cfg2"]["lo"], CONFIGS["cfg2"]["hi"], 202)
    queries = sa.SequenceStore.from_sequences(query_seqs)
    cells = db_len * sum(len(q) for q in query_seqs)
    k = 64
    d_rect = torch.empty(m * n, dtype=torch.int32, device="cuda")
    d_vrect = torch.empty(m * n, dtype=torch.int32, device="cuda")
    with sa.SearchContext(db, queries, scoring, 0) as sx:
        d_scratch = torch.empty(sx.search_scratch_bytes(0, m) // 4, dtype=torch.int32, device="cuda")
        d_den = torch.empty(n + m, dtype=torch.int32, device="cuda")
        d_hits = torch.empty(3 * m * k, dtype=torch.int32, device="cuda")
        d_part = torch.empty(max(sa.hits_scratch_bytes(n, m, k) // 4, 1), dtype=torch.int32, device="cuda")
        sr = median_ms(stream, lambda: sx.search_range(0, m, d_rect.data_ptr(), d_scratch.data_ptr(), stream=s))
        sx.timing(True)
        for _ in range(reps):
            sx.search_range(0, m, d_rect.data_ptr(), d_scratch.data_ptr(), stream=s)
        stream.synchronize()
        t = sx.timing_read()
        sx.timing(False)
        align_ms = t["all_kernels_ms"] / reps
        say(f"\nM = {m}: {m * n} pairs, {cells} cells; search_range {sr[0]:.3f} ms ({sr[1]:.3f} .. {sr[2]:.3f}); its alignment kernels {align_ms:.3f} ms "
            f"(mean of {reps}) = {cells / (align_ms * 1e-3) / 1e12:.3f} T cells/s")
        den = median_ms(stream, lambda: sx.denominators(sa.NORM_SELF, d_den.data_ptr(), stream=s))
        swp = median_ms(stream, lambda: sx.normalize_rect(d_rect.data_ptr(), m, 0, d_den.data_ptr(), sa.NORM_MIN, d_vrect.data_ptr(), stream=s))
        inp = median_ms(stream, lambda: sx.normalize_rect(d_vrect.data_ptr(), m, 0, d_den.data_ptr(), sa.NORM_MEAN, d_vrect.data_ptr(), stream=s))
        sx.normalize_rect(d_rect.data_ptr(), m, 0, d_den.data_ptr(), sa.NORM_MIN, d_vrect.data_ptr(), stream=s)
        hit = median_ms(stream, lambda: sx.hits(d_vrect.data_ptr(), m, k, d_hits.data_ptr(), d_hits.data_ptr() + 4 * m * k, d_part.data_ptr(), stream=s))
        tak = median_ms(stream, lambda: sx.hits_take(d_rect.data_ptr(), m, k, d_hits.data_ptr(), d_hits.data_ptr() + 8 * m * k, stream=s))
        total = den[0] + swp[0] + tak[0]
        say(f"  normalised (self-min): denominators of {n + m} sequences {den[0]:.3f} ms ({den[1]:.3f} .. {den[2]:.3f}); sweep {swp[0]:.3f} ms "
            f"({swp[1]:.3f} .. {swp[2]:.3f}), in place (mean) {inp[0]:.3f} ms; take, k = {k}, {tak[0]:.3f} ms ({tak[1]:.3f} .. {tak[2]:.3f}); "
            f"hits on the value rectangle {hit[0]:.3f} ms")
        say(f"  denominators + sweep + take = {total:.3f} ms = {100.0 * total / align_ms:.2f} % of the alignment beside it; the sweep moves 8 M N bytes: "
            f"{8.0 * m * n / (swp[0] * 1e-3) / ROOF:.3f} of the 8 TB/s roof (in place {8.0 * m * n / (inp[0] * 1e-3) / ROOF:.3f})")
        if m == 1000:
            verdicts.append(f"condition (M = 1000: denominators + sweep + take <= 10 % of the alignment beside it): {total:.3f} ms of {align_ms:.3f} ms = "
                            f"{100.0 * total / align_ms:.2f} % -> {'MET' if total <= 0.10 * align_ms else 'MISSED'}")
        # identity: the rectangle form, score and pid together, and the triangle form over the same number of pairs of the same
        # (concatenated) store -- the three sweeps take turns run by run, so that a drift of the clocks meets them alike
        cat = sa.SequenceStore.from_sequences(list(db_seqs) + list(query_seqs))
        with sa.Context(cat, scoring, 0) as cx:
            count = m * n
            ranges = (("[0, M N)", 0), ("[tri(N), + M N)", n * (n - 1) // 2))
            sweeps = [lambda: sx.identity_rect(0, m, score=d_rect.data_ptr(), pid=d_vrect.data_ptr(), denom=sa.PID_COLUMNS, stream=s)]
            for _, start in ranges:
                sweeps.append(lambda start=start: cx.identity_range(start, count, score=d_rect.data_ptr(), pid=d_vrect.data_ptr(), denom=sa.PID_COLUMNS, stream=s))
            rect_t, *tri_ts = median_ms_in_turns(stream, sweeps)
            tri_cells = [cx.cells(start, count) for _, start in ranges]
    rect_rate = cells / (rect_t[0] * 1e-3)
    say(f"  identity, rectangle form: {rect_t[0]:.3f} ms ({rect_t[1]:.3f} .. {rect_t[2]:.3f}, spread {100 * spread(rect_t):.2f} %) = {rect_rate / 1e9:.2f} G cells/s; "
        f"identity sweep / packed alignment of the same rectangle: {rect_t[0] / align_ms:.1f} x (not judged)")
    for (what, _), tri_t, c in zip(ranges, tri_ts, tri_cells):
        tri_rate = c / (tri_t[0] * 1e-3)
        tol = max(spread(rect_t), spread(tri_t))
        say(f"  triangle form over pairs {what} of the concatenated store, {c} cells: {tri_t[0]:.3f} ms ({tri_t[1]:.3f} .. {tri_t[2]:.3f}, "
            f"spread {100 * spread(tri_t):.2f} %) = {tri_rate / 1e9:.2f} G cells/s; rectangle / triangle per cell: {rect_rate / tri_rate:.4f}")
        verdicts.append(f"condition (M = {m}: the rectangle form no slower per cell than the triangle form over {what} by more than the spread, "
                        f"{100 * tol:.2f} %): {rect_rate / tri_rate:.4f} -> {'MET' if rect_rate >= tri_rate * (1.0 - tol) else 'MISSED'}")
    del d_rect, d_vrect
say()
for v in verdicts:
    say(v)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
