"""tools/dev/search_strands_time.py [--reps R] [--out FILE] [--db N] [--small] -- the two-strand search (csrc/sa_strands.hip) measured two ways.  Writes
what it prints to FILE (default profiles/search_strands_time.txt).

1. The whole call against the existing code path.  sa_hip_search_strands at k = 8 and k = 64 on the shape of config 4 (SW, NUC.4.4,
   gaps 10 / 1, reads of 120 - 180 bp): a database of 30 000 reads, queries M = 3 and M = 4096 -- mutated pieces of database reads,
   every second one reverse-complemented.  Beside it the sum of two sa_hip_search calls on the same inputs: the queries as given,
   and a reverse complement made on the host (sa_reverse_complement).  Both are host in / host out and synchronous, so the host clock
   around a call is the call; the device seconds are the library's own (sa_hip_last_search_*).  The two versions ALTERNATE, R times
   (default 7) after one warm-up each; median (min .. max), the ratio of the medians, and the run-to-run spread of each version as
   (max - min) / median -- a ratio inside that spread is no difference.

2. The fold against the HBM roof.  sa_ctx_strand_fold on device rectangles of random int32 (the fold does not care where values come
   from; the context's sequences are single residues), HIP events on one stream, two warm-ups, median of R.  Shapes (M, N) as
   tools/dev/search_above_time.py has them: (3, 10^6), (1000, 10^5), (20 000, 5 000).  Bytes every pass must move, against the 8 TB/s
   roof the other *_time.py tools use: 12 + 1/8 per cell by raw score (two reads, one write, one bit), 24 + 1/8 with the raw scores
   carried along; in place the same bytes."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import sequencealigner_amd as sa  # noqa: E402
from tests.synth import make_dna_set  # noqa: E402

ROOF = 8e12
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "search_strands_time.txt")
n_db = int(sys.argv[sys.argv.index("--db") + 1]) if "--db" in sys.argv else 30_000
shapes = [(3, 1_000_000), (1000, 100_000), (20_000, 5_000)]
if "--small" in sys.argv:  # (a rehearsal of the tool itself)
    n_db, shapes = 300, [(3, 1000), (40, 500)]
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(times):
    return (max(times) - min(times)) / statistics.median(times)


def three(times, unit=1e3):
    return f"{statistics.median(times) * unit:.3f} ({min(times) * unit:.3f} .. {max(times) * unit:.3f})"


say(f"device: {sa.device_name(0)}; {reps} runs after warm-up, median (min .. max); roof {ROOF / 1e12:.0f} TB/s")

# ---- 1. the whole call against two plain searches ----------------------------------------------------------------------------------
scoring = sa.Scoring.from_names("sw", "nuc44", gap_open=10, gap_extend=1)
reads = make_dna_set(n_db, 120, 180, 4)
db = sa.SequenceStore.from_sequences(reads)
say(f"\n1. sa_hip_search_strands against sa_hip_search + sa_hip_search (forward, host-made reverse complement): SW, NUC.4.4, 10 / 1, "
    f"N = {n_db} reads of 120 - 180 bp; milliseconds of host clock around the calls, the versions alternating")
for m in (3, 4096 if n_db >= 30_000 else 64):
    rng = np.random.default_rng(m)
    qs = []
    for t in range(m):
        b = bytearray(reads[int(rng.integers(0, n_db))])
        for p in np.flatnonzero(rng.random(len(b)) < 0.05):
            b[p] = b"ACGT"[int(rng.integers(0, 4))]
        qs.append(bytes(b))
    fwd = sa.SequenceStore.from_sequences(qs)
    rev = sa.reverse_complement(fwd, scoring=scoring)
    queries = sa.SequenceStore.from_sequences([rev.sequence(t) if t % 2 else qs[t] for t in range(m)])
    queries_rc = sa.reverse_complement(queries, scoring=scoring)
    for k in (8, 64):
        both_t, two_t, both_dev, two_dev, fold_dev = [], [], [], [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            got = sa.hip_search_strands(db, queries, scoring, k=k)
            t1 = time.perf_counter()
            dev_a = sa.last_search_seconds() + sa.last_search_strands_seconds()
            fold = sa.last_search_strands_seconds()
            batches = sa.last_search_breakdown()["batches"]
            t2 = time.perf_counter()
            a = sa.hip_search(db, queries, scoring, k=k)
            dev_b = sa.last_search_seconds()
            b = sa.hip_search(db, queries_rc, scoring, k=k)
            dev_b += sa.last_search_seconds()
            t3 = time.perf_counter()
            if rep == 0:  # (warm-up; and the fold is the host's merge of the two plain searches)
                strand = got[3].astype(bool)
                assert np.array_equal(got[1][:, 0], np.maximum(a[1][:, 0], b[1][:, 0])), "the best folded hit is the better of the two best"
                say(f"  M = {m}, k = {k}: {int(strand.sum())} of {strand.size} hits on the reverse strand; {batches} batch(es)")
                continue
            both_t.append(t1 - t0)
            two_t.append(t3 - t2)
            both_dev.append(dev_a)
            two_dev.append(dev_b)
            fold_dev.append(fold)
        ratio, dev_ratio = statistics.median(both_t) / statistics.median(two_t), statistics.median(both_dev) / statistics.median(two_dev)
        say(f"    one call, both strands   {three(both_t)} ms, spread {100 * spread(both_t):.1f} %; device {three(both_dev)} ms of which fold + strand take "
            f"{three(fold_dev)} ms")
        say(f"    two plain searches, sum  {three(two_t)} ms, spread {100 * spread(two_t):.1f} %; device {three(two_dev)} ms")
        say(f"    ratio of the medians     {ratio:.3f} (host clock), {dev_ratio:.3f} (device time)")

# ---- 2. the fold against the roof --------------------------------------------------------------------------------------------------
stream = torch.cuda.Stream()


def median_ms(fn, warm=2):
    times = []
    for rep in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        if rep >= warm:
            times.append(e0.elapsed_time(e1) * 1e-3)
    return times


say("\n2. sa_ctx_strand_fold on device rectangles, HIP events on one stream; bytes per cell: 12 + 1/8 by raw score, 24 + 1/8 with the scores carried")
tiny = sa.Scoring.from_names("nw", "nuc44", gap_pen=4)
for m, n in shapes:
    one = [b"ACGT"[t % 4:t % 4 + 1] for t in range(8)]
    dbs = sa.SequenceStore.from_sequences([one[t % 8] for t in range(n)])
    qss = sa.SequenceStore.from_sequences([one[t % 8] for t in range(m)])
    cells, words = m * n, sa.strand_words(n)
    with sa.SearchContext(dbs, qss, tiny, 0, strands=True) as sx:
        gen = torch.Generator(device="cuda").manual_seed(m + n)
        bufs = [torch.randint(-2**31, 2**31 - 1, (cells,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32) for _ in range(4)]
        vf, vr, sf, sr = (b.data_ptr() for b in bufs)
        outs = [torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(2)]
        vb, sb = (o.data_ptr() for o in outs)
        bits = torch.empty(m * words, dtype=torch.int64, device="cuda")
        s = stream.cuda_stream
        raw = median_ms(lambda: sx.strand_fold(vf, vr, m, vb, bits.data_ptr(), stream=s))
        carried = median_ms(lambda: sx.strand_fold(vf, vr, m, vb, bits.data_ptr(), d_sfwd_ptr=sf, d_srev_ptr=sr, d_sbest_ptr=sb, stream=s))
        nobits = median_ms(lambda: sx.strand_fold(vf, vr, m, vb, 0, stream=s))
        # (in place last: it overwrites the forward rectangles; the bytes moved do not depend on the values)
        in_place = median_ms(lambda: sx.strand_fold(vf, vr, m, vf, bits.data_ptr(), d_sfwd_ptr=sf, d_srev_ptr=sr, d_sbest_ptr=sf, stream=s))
        segs = max(1, min((8192 + m - 1) // m, n // 64)) if m < 2048 else 1
        say(f"  (M, N) = ({m}, {n}): {cells} cells, {segs} segment(s) per row = {m * segs} waves")
        for name, times, per in (("by raw score", raw, 12.125), ("by raw score, no bitmap", nobits, 12.0), ("scores carried", carried, 24.125),
                                 ("scores carried, in place", in_place, 24.125)):
            med = statistics.median(times)
            say(f"    {name:<26s} {three(times)} ms = {per * cells / med / 1e9:8.1f} GB/s = {per * cells / med / ROOF:.3f} of the roof")
        k = min(64, n)
        index = torch.randint(0, n, (m * k,), dtype=torch.int32, device="cuda", generator=gen)
        strand = torch.empty(m * k, dtype=torch.uint8, device="cuda")
        take = median_ms(lambda: sx.hits_strand(bits.data_ptr(), m, k, index.data_ptr(), strand.data_ptr(), stream=s))
        say(f"    sa_ctx_hits_strand, k = {k:<5d}  {three(take)} ms")
        del bufs, outs, bits, index, strand
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
