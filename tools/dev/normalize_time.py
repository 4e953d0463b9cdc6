"""tools/dev/normalize_time.py [--reps R] -- the normalised scores (sa_ctx_denominators + sa_ctx_normalize,
csrc/sa_normalize.hip) beside the alignment that feeds them, all device-resident and timed with HIP events on one stream: a few
warm-up runs, then the median of R (default 11).

Store: config 2 (10 000 proteins, P = 49 995 000 pairs).  The self-scores (sa_k_self, one wavefront per sequence), the lengths,
the sweep (sa_k_normalize: 4 P bytes read, 4 P bytes written) out of place and in place for the three rules, with their share of
the alignment ms of the same store in the same process, and the sweep's 8 P bytes / time as a fraction of the 8 TB/s HBM roof.
The answers are checked before anything is timed: the self-scores against the matrix entry of a sequence and its copy (a store
of the first 200 sequences, doubled), the sweep against torch's int64 floor division of the same device matrix.

Condition (config 2): denominators (self-scores) + sweep together take no more than 10 % of the alignment measured beside them."""
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


seqs, cfg2 = make_config("cfg2")
scoring = sa.Scoring.from_names(cfg2["method"], cfg2["matrix"], **cfg2["gaps"])
print(f"device: {sa.device_name(0)}; HIP events on one stream, {reps} runs after 3 warm-ups, median (min .. max)")
print(f"roof: {ROOF / 1e12:.0f} TB/s")
stream = torch.cuda.Stream()
s = stream.cuda_stream

# the self-scores, checked: entry (i, 200 + i) of the matrix of a doubled store is sequence i against itself
half = seqs[:200]
twice = sa.SequenceStore.from_sequences(half + half)
full = torch.from_numpy(sa.hip_align(twice, scoring, triangular=False))
d_check = torch.empty(400, dtype=torch.int32, device="cuda")
with sa.Context(twice, scoring, 0) as ctx:
    ctx.denominators(sa.NORM_SELF, d_check.data_ptr(), stream=s)
    stream.synchronize()
assert torch.equal(d_check[:200].cpu(), full[torch.arange(200), 200 + torch.arange(200)]), "self-scores differ from the matrix entries"

store = sa.SequenceStore.from_sequences(seqs)
n, pairs = store.num, store.pairs
d_packed = torch.empty(pairs, dtype=torch.int32, device="cuda")
d_out = torch.empty(pairs, dtype=torch.int32, device="cuda")
d_den = torch.empty(n, dtype=torch.int32, device="cuda")
d_len = torch.empty(n, dtype=torch.int32, device="cuda")
jj = torch.repeat_interleave(torch.arange(1, n, device="cuda"), torch.arange(1, n, device="cuda"))
ii = torch.arange(pairs, device="cuda") - jj * (jj - 1) // 2
with sa.Context(store, scoring, 0) as ctx:
    p, o, d = d_packed.data_ptr(), d_out.data_ptr(), d_den.data_ptr()
    align_ms, lo, hi = median_ms(stream, lambda: ctx.align_range(0, pairs, p, stream=s), warm=2)
    print(f"\nconfig 2: N = {n}, P = {pairs} pairs ({4 * pairs / 1e6:.0f} MB); alignment (sa_ctx_align_range) {align_ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
    self_ms, lo, hi = median_ms(stream, lambda: ctx.denominators(sa.NORM_SELF, d, stream=s))
    print(f"  self-scores (sa_k_self)      {self_ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * self_ms / align_ms:5.2f} % of the alignment")
    len_ms, lo, hi = median_ms(stream, lambda: ctx.denominators(sa.NORM_LENGTH, d_len.data_ptr(), stream=s))
    print(f"  lengths (sa_k_lengths)       {len_ms:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    assert d_len.cpu().tolist() == [len(q) for q in seqs]
    di, dj = d_den.long()[ii], d_den.long()[jj]
    sweep = {}
    for rule, name in ((sa.NORM_MIN, "min"), (sa.NORM_MAX, "max"), (sa.NORM_MEAN, "mean")):
        ctx.normalize(p, d, rule, o, stream=s)
        stream.synchronize()
        den = torch.minimum(di, dj) if rule == sa.NORM_MIN else torch.maximum(di, dj) if rule == sa.NORM_MAX else di + dj
        num = d_packed.long() * sa.NORM_SCALE * (2 if rule == sa.NORM_MEAN else 1)
        want = torch.div(num, den, rounding_mode="floor").clamp(-2**31, 2**31 - 1).int()
        assert int(den.min().item()) > 0 and torch.equal(d_out, want), f"sweep ({name}) differs from torch's floor division"
        del den, num, want
        ms, lo, hi = median_ms(stream, lambda: ctx.normalize(p, d, rule, o, stream=s))
        sweep[name] = ms
        print(f"  sweep, {name:4s} (sa_k_normalize) {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * ms / align_ms:5.2f} % of the alignment;  "
              f"8 P bytes / time = {8.0 * pairs / (ms * 1e-3) / ROOF:.3f} of the roof")
    # in place: the matrix is rewritten every run, which changes the values but not the work
    ms, lo, hi = median_ms(stream, lambda: ctx.normalize(o, d, sa.NORM_MIN, o, stream=s))
    print(f"  sweep, min, in place         {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  8 P bytes / time = {8.0 * pairs / (ms * 1e-3) / ROOF:.3f} of the roof")
    both_ms, lo, hi = median_ms(stream, lambda: (ctx.denominators(sa.NORM_SELF, d, stream=s), ctx.normalize(p, d, sa.NORM_MIN, o, stream=s)))
    print(f"  self-scores + sweep (min)    {both_ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  = {100.0 * both_ms / align_ms:5.2f} % of the alignment")
print(f"\ncondition (config 2: denominators + sweep <= 10 % of the alignment beside them): {both_ms:.3f} ms of "
      f"{align_ms:.3f} ms = {100.0 * both_ms / align_ms:.2f} % -> {'MET' if both_ms <= 0.10 * align_ms else 'MISSED'}")
