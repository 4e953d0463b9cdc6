"""tools/dev/fit_time.py [--reps R] [--out FILE] -- what fitting the queries inside the database sequences costs (csrc/sa_fit.hip),
beside the identity sweep of the same rectangle (sa_ctx_identity_rect: the same pair-per-wave sweep with a payload of two words
instead of three and no end-cell bookkeeping) and beside the packed alignment of the same rectangle (sa_ctx_search_range), all in
one process, device-resident and timed with HIP events on one stream: two warm-up runs, then the median of R (default 5); the
sweeps take turns run by run.  The report goes to FILE (default profiles/fit_time.txt) and to stdout.

Two rectangles of 64 queries of 150 residues against 20 000 entries of 300 - 1000 residues: DNA (NW / nuc44 / 4) and protein
(Gotoh / BLOSUM62 / 10-1).  Per rectangle: sa_ctx_fit_rect with the score alone and with all six outputs, per DP cell; the list
pass (sa_ctx_fit_pairs) over the 64 x 8 hits; the fitted alignments of those hits (fill + walk).  No pass mark: the ratios are
what DESIGN 4.21 quotes."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_dna_set, make_protein_set  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fit_time.txt")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def median_ms_in_turns(stream, fns, warm=2):
    """several calls that take turns: run 1 of each, run 2 of each, ..."""
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


N, M, K = 20_000, 64, 8
stream = torch.cuda.Stream()
s = stream.cuda_stream
say(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 2 warm-ups, the sweeps taking turns, median (min .. max)")
for name, make, scoring in (("DNA", make_dna_set, sa.Scoring.from_names("nw", "nuc44", gap_pen=4)),
                            ("protein", make_protein_set, sa.Scoring.from_names("ga", "blosum62", gap_open=10, gap_extend=1))):
    db_seqs, query_seqs = make(N, 300, 1000, 301), make(M, 150, 150, 302)
    for q in range(0, M, 2):  # half the queries are reads of an entry
        src = db_seqs[(q * 311) % N]
        query_seqs[q] = src[100:250]
    db, queries = sa.SequenceStore.from_sequences(db_seqs), sa.SequenceStore.from_sequences(query_seqs)
    cells = sum(len(x) for x in db_seqs) * sum(len(x) for x in query_seqs)
    bufs = [torch.empty(M * N, dtype=torch.int32, device="cuda") for _ in range(6)]
    p = [b.data_ptr() for b in bufs]
    with sa.SearchContext(db, queries, scoring, 0) as sx:
        d_scratch = torch.empty(sx.search_scratch_bytes(0, M) // 4 + 2, dtype=torch.int32, device="cuda")
        sweeps = [lambda: sx.fit_rect(0, M, score=p[0], stream=s),
                  lambda: sx.fit_rect(0, M, score=p[0], db_begin=p[1], db_end=p[2], identities=p[3], columns=p[4], pid=p[5], denom=sa.PID_SHORTER, stream=s),
                  lambda: sx.identity_rect(0, M, score=p[0], identities=p[3], columns=p[4], pid=p[5], denom=sa.PID_SHORTER, stream=s),
                  lambda: sx.search_range(0, M, p[1], d_scratch.data_ptr(), stream=s)]
        fit1, fit6, ident, packed = median_ms_in_turns(stream, sweeps)
        say(f"\n{name}: {M} queries of 150 residues against {N} entries of 300 - 1000, {scoring.method and 'Gotoh' or 'NW'}; {M * N} pairs, {cells} cells")
        for what, t in (("sa_ctx_fit_rect, score alone", fit1), ("sa_ctx_fit_rect, all six outputs", fit6), ("sa_ctx_identity_rect, four outputs", ident),
                        ("sa_ctx_search_range (packed kernels)", packed)):
            say(f"  {what:<40s} {t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f}, spread {100 * spread(t):.2f} %) = {cells / (t[0] * 1e-3) / 1e9:8.2f} G cells/s")
        say(f"  fit (all outputs) / identity sweep: {fit6[0] / ident[0]:.3f}; fit (score alone) / identity sweep: {fit1[0] / ident[0]:.3f}; "
            f"fit (score alone) / packed rectangle: {fit1[0] / packed[0]:.1f} x")
        # the hits of the fit rectangle, then the list pass and the fitted alignments over them
        sx.fit_rect(0, M, score=p[0], stream=s)
        d_hits = torch.empty(2 * M * K, dtype=torch.int32, device="cuda")
        d_part = torch.empty(max(sa.hits_scratch_bytes(N, M, K) // 4, 1) + 2, dtype=torch.int32, device="cuda")
        sx.hits(p[0], M, K, d_hits.data_ptr(), d_hits.data_ptr() + 4 * M * K, d_part.data_ptr(), stream=s)
        stream.synchronize()
        index = d_hits[:M * K].cpu().numpy()
        d_query = torch.from_numpy(np.repeat(np.arange(M, dtype=np.int32), K)).cuda()
        hit_cells = sum(len(db_seqs[d]) * 150 for d in index)
        (lst,) = median_ms_in_turns(stream, [lambda: sx.fit_pairs(d_query.data_ptr(), d_hits.data_ptr(), M * K, score=p[0], db_begin=p[1], db_end=p[2], stream=s)])
        say(f"  list pass over the {M} x {K} hits (score, db_begin, db_end), {hit_cells} cells: {lst[0]:.3f} ms ({lst[1]:.3f} .. {lst[2]:.3f})")
        pairs = [(t // K, int(d)) for t, d in enumerate(index)]
        fills, walks = [], []
        for rep in range(2 + reps):
            sx.fit_alignments(pairs)
            if rep >= 2:
                bd = sa.last_alignments_breakdown()
                fills.append(bd["fill_seconds"] * 1e3)
                walks.append(bd["walk_seconds"] * 1e3)
        say(f"  fitted alignments of the same hits: fill {statistics.median(fills):.3f} ms ({min(fills):.3f} .. {max(fills):.3f}), "
            f"walk + scan + compaction {statistics.median(walks):.3f} ms ({min(walks):.3f} .. {max(walks):.3f})")
    del bufs
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
