"""GPU (-m gpu): alignments for chosen pairs traced back on the device (sa_ctx_alignments / sa_hip_alignments,
csrc/sa_traceback.hip; the tool's --alignments).  The contract is in include/seqalign_hip.h.

1. exact contract: records and CIGARs equal tests/traceback_ref.py (plain Python over full tables), field by field
2. anchored at the reference, independent of the tie rule: score == the oracle's, the CIGAR re-scored by the documented rule
   equals the score, lengths / spans / identities / run structure are consistent -- for every pair, none left out
3. batching: the batch-bytes switch forcing >= 4 batches gives the same bytes as the default
4. determinism: twice the same bytes; duplicates and a shuffled list give per-pair results equal to the sorted list's
5. the tool: seqalign -k 5 --alignments, with and without --neighbors-only"""
import subprocess

import numpy as np
import pytest

from tests import traceback_ref
from tests.synth import make_dna_set, make_protein_set

pytestmark = pytest.mark.gpu

GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end", "columns", "identities")


def both_orders(n: int, count: int, seed: int) -> np.ndarray:
    """`count` pairs (a, b), a != b, of n sequences: about half with a > b"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, count)
    b = (a + 1 + rng.integers(0, n - 1, count)) % n
    return np.stack([a, b], axis=1).astype(np.int32)


def per_pair(alns, t):
    """record t as a plain tuple + its runs: what has to be equal between two calls whatever the pair's place in the list"""
    r = alns.records[t]
    return tuple(int(r[f]) for f in FIELDS), tuple(alns.runs(t))


# ---- 1. exact contract --------------------------------------------------------------------------------------------------------
def tie_heavy_sequences():
    seqs = [b"A" * k for k in (1, 2, 7, 33, 64, 65, 80)]                      # homopolymers: every tie exists
    seqs += [b"W" * 40, b"AW" * 30, b"WA" * 35, b"ARND" * 20, b"DNRA" * 19]   # repeats, a pair that shares nothing (A vs W)
    seqs += [b"A", b"W", b"R"]                                               # length 1
    return seqs


CONTRACT_SCORINGS = [
    ("nw", "blosum62", dict(gap_pen=4)), ("ga", "blosum62", dict(gap_open=10, gap_extend=1)), ("sw", "blosum62", dict(gap_open=10, gap_extend=1)),
    ("nw", "blosum62", dict(gap_pen=0)), ("ga", "blosum62", dict(gap_open=0, gap_extend=0, equal_affine_to_nw=False)), ("sw", "blosum62", dict(gap_open=0, gap_extend=0)),
    ("sw", "blosum62", dict(gap_open=4, gap_extend=4)),   # open == extend (Gotoh with equal gaps becomes NW: the reference's rule)
    ("ga", "blosum62", dict(gap_open=3, gap_extend=7)), ("sw", "pam250", dict(gap_open=2, gap_extend=5)),   # |open| < |extend|
]


@pytest.mark.parametrize("method,matrix,gaps", CONTRACT_SCORINGS, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_records_and_cigars_equal_the_python_restatement(method, matrix, gaps, sa):
    seqs = make_protein_set(40, 1, 80, 11) + tie_heavy_sequences()
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, matrix, **gaps)
    n = store.num
    tie0 = 40
    heavy = [(a, b) for a in range(tie0, n) for b in range(tie0, n) if a != b]     # every ordered pair of the tie-heavy ones
    pairs = np.concatenate([both_orders(n, 150, 5), np.array(heavy, np.int32)])
    got = sa.hip_alignments(store, scoring, pairs)
    assert len(got.records) == len(pairs) and got.records["cigar_off"][0] == 0
    assert np.array_equal(got.records["cigar_off"][1:], np.cumsum(got.records["cigar_len"].astype(np.int64))[:-1])
    assert int(got.records["cigar_off"][-1]) + int(got.records["cigar_len"][-1]) == len(got.cigar)
    empty = 0
    for t, (a, b) in enumerate(pairs):
        want = traceback_ref.align_pair(scoring, seqs[a], seqs[b], int(a), int(b))
        have = {f: int(got.records[t][f]) for f in FIELDS}
        have["cigar"] = got.runs(t)
        assert have == want, f"{method} pair {t} = ({a}, {b}), lengths {len(seqs[a])} x {len(seqs[b])}:\n got  {have}\n want {want}"
        empty += want["columns"] == 0
    assert scoring.method == {"nw": 0, "ga": 1, "sw": 2}[method]
    if method == "sw" and gaps.get("gap_open"):
        assert empty >= 2   # A-only against W-only, both orders: best 0, the empty alignment


# ---- 2. anchored at the reference, independent of the tie rule ---------------------------------------------------------------------
def check_against_oracle(sa, oracle, seqs, scoring, pairs):
    """every property the contract states that does not depend on how ties are broken; returns the number of pairs checked"""
    store = sa.SequenceStore.from_sequences(seqs)
    got = sa.hip_alignments(store, scoring, pairs)
    lo, hi = pairs.min(axis=1).astype(np.int64), pairs.max(axis=1).astype(np.int64)
    want_score = oracle.align_pairs(store, scoring, hi * (hi - 1) // 2 + lo)
    print(f"  {scoring.method_name} {scoring.matrix_name}: {len(pairs)} pairs, {got.records['columns'].sum()} columns, "
          f"{len(got.cigar)} runs, device {sa.last_alignments_seconds() * 1e3:.3f} ms")
    assert np.array_equal(got.records["score"], want_score)
    sub = scoring.sub.reshape(24, 24)
    g, o, e = scoring.gap_pen, scoring.gap_opn, scoring.gap_ext
    nw = scoring.method == 0
    checked = 0
    for t, (a, b) in enumerate(pairs):
        r = got.records[t]
        runs = got.runs(t)
        sa_, sb_ = seqs[a], seqs[b]
        # the re-scorer: S over the M columns in the library's orientation (rows = min(a, b)), a cost per gap run
        total, i, j = 0, int(r["a_begin"]), int(r["b_begin"])
        for length, op in runs:
            if op == "M":
                for k in range(length):
                    ca, cb = int(scoring.lut[sa_[i + k]]), int(scoring.lut[sb_[j + k]])
                    lo_c, hi_c = (ca, cb) if a < b else (cb, ca)
                    total += int(sub[lo_c, hi_c] if nw else sub[hi_c, lo_c])
                i, j = i + length, j + length
            else:
                total += length * g if nw else o + (length - 1) * max(o, e)
                i, j = (i + length, j) if op == "I" else (i, j + length)
        assert total == int(r["score"]), f"pair {t} = ({a}, {b}): the CIGAR scores {total}, the record says {r['score']}"
        assert (i, j) == (int(r["a_end"]), int(r["b_end"]))
        assert sum(length for length, _ in runs) == int(r["columns"]) and all(length > 0 for length, _ in runs)
        assert sum(length for length, op in runs if op != "D") == int(r["a_end"]) - int(r["a_begin"])
        assert sum(length for length, op in runs if op != "I") == int(r["b_end"]) - int(r["b_begin"])
        assert all(x[1] != y[1] for x, y in zip(runs, runs[1:])), "adjacent runs share an op"
        ga, gb = got.aligned(t, store)
        assert len(ga) == len(gb) == int(r["columns"])
        assert sum(x == y and x != "-" for x, y in zip(ga, gb)) == int(r["identities"])
        assert ga.replace("-", "").encode() == sa_[int(r["a_begin"]):int(r["a_end"])] and gb.replace("-", "").encode() == sb_[int(r["b_begin"]):int(r["b_end"])]
        if scoring.method == 2:
            assert 0 <= r["a_begin"] <= r["a_end"] <= len(sa_) and 0 <= r["b_begin"] <= r["b_end"] <= len(sb_)
            if runs:  # the walk stops on M == 0 and best > 0 is reached on a diagonal step
                assert runs[0][1] == "M" and runs[-1][1] == "M"
            else:
                assert int(r["score"]) == 0 and (r["a_begin"], r["a_end"], r["b_begin"], r["b_end"]) == (0, 0, 0, 0)
        else:
            assert (r["a_begin"], r["a_end"], r["b_begin"], r["b_end"]) == (0, len(sa_), 0, len(sb_))
        checked += 1
    return checked


@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
@pytest.mark.parametrize("matrix", ["blosum62", "pam250"])
def test_proteins_anchored_at_the_oracle(method, matrix, sa, oracle):
    scoring = sa.Scoring.from_names(method, matrix, **GAPS[method])
    seqs = make_protein_set(150, 20, 190, 3) + make_protein_set(60, 200, 380, 4)
    pairs = both_orders(len(seqs), 500, 9)
    assert (pairs[:, 0] > pairs[:, 1]).sum() > 100 and (pairs[:, 0] < pairs[:, 1]).sum() > 100
    assert check_against_oracle(sa, oracle, seqs, scoring, pairs) == len(pairs)   # no pair left out


@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_long_sequences_anchored_at_the_oracle(method, sa, oracle):
    """1000 - 3000 residues: dozens of strips, the boundary column, a pair's scratch of several megabytes"""
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    seqs = make_protein_set(6, 1000, 3000, 21) + make_protein_set(10, 30, 400, 22)
    pairs = both_orders(len(seqs), 40, 13)
    assert check_against_oracle(sa, oracle, seqs, scoring, pairs) == len(pairs)


@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_dna_anchored_at_the_oracle(method, sa, oracle):
    gaps = dict(gap_pen=8) if method == "nw" else dict(gap_open=16, gap_extend=4)
    scoring = sa.Scoring.from_names(method, "dnafull", **gaps)
    seqs = make_dna_set(120, 20, 300, 6, iupac=True)
    pairs = both_orders(len(seqs), 400, 17)
    assert check_against_oracle(sa, oracle, seqs, scoring, pairs) == len(pairs)


# ---- 3. batching ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
def test_forced_batches_give_the_same_bytes(method, sa, monkeypatch):
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    seqs = make_protein_set(200, 20, 300, 8)
    store = sa.SequenceStore.from_sequences(seqs)
    pairs = both_orders(len(seqs), 600, 23)
    monkeypatch.delenv("SA_HIP_TRACE_BATCH_BYTES", raising=False)
    whole = sa.hip_alignments(store, scoring, pairs)
    assert sa.last_alignments_breakdown()["batches"] == 1
    for cap in (4 << 20, 1):   # a few megabytes: a handful of batches; one byte: every pair is its own batch
        monkeypatch.setenv("SA_HIP_TRACE_BATCH_BYTES", str(cap))
        cut = sa.hip_alignments(store, scoring, pairs)
        batches = sa.last_alignments_breakdown()["batches"]
        assert batches >= 4 and (cap > 1 or batches == len(pairs)), batches
        assert cut.records.tobytes() == whole.records.tobytes() and cut.cigar.tobytes() == whole.cigar.tobytes()


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------
def test_same_bytes_twice_and_order_of_the_list_does_not_matter(sa):
    scoring = sa.Scoring.from_names("sw", "blosum62", gap_open=10, gap_extend=1)
    seqs = make_protein_set(120, 10, 200, 12)
    store = sa.SequenceStore.from_sequences(seqs)
    pairs = both_orders(len(seqs), 400, 31)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    sorted_pairs = pairs[order]
    with sa.Context(store, scoring) as ctx:
        first = ctx.alignments(sorted_pairs)
        second = ctx.alignments(sorted_pairs)
        assert first.records.tobytes() == second.records.tobytes() and first.cigar.tobytes() == second.cigar.tobytes()
        expected = {tuple(p): per_pair(first, t) for t, p in enumerate(sorted_pairs.tolist())}
        shuffled = ctx.alignments(pairs)
        for t, p in enumerate(pairs.tolist()):
            assert per_pair(shuffled, t) == expected[tuple(p)]
        doubled = np.concatenate([pairs[:50], pairs[:50][::-1], pairs[:50]])
        dup = ctx.alignments(doubled)
        for t, p in enumerate(doubled.tolist()):
            assert per_pair(dup, t) == expected[tuple(p)]
        assert len(ctx.alignments(np.zeros((0, 2), np.int32)).records) == 0   # npairs == 0: a valid empty result
        # the context still computes scores afterwards
    via_hip = sa.hip_alignments(store, scoring, sorted_pairs)
    assert via_hip.records.tobytes() == first.records.tobytes() and via_hip.cigar.tobytes() == first.cigar.tobytes()


def test_bad_pairs_raise_and_the_process_lives_on(sa):
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    store = sa.SequenceStore.from_sequences(make_protein_set(10, 10, 30, 2))
    for bad, message in (([(3, 3)], "a == b"), ([(0, 10)], "out of range"), ([(-1, 2)], "out of range")):
        with pytest.raises(sa.AlignError, match=message):
            sa.hip_alignments(store, scoring, bad)
    assert sa.hip_alignments(store, scoring, [(0, 1)]).cigar_string(0) != ""


# ---- 5. the tool -------------------------------------------------------------------------------------------------------------------
def h5_typed(path, name: str, dtype: str) -> np.ndarray:
    from tests.host_binding import H5DUMP
    out = path.with_name(path.name + "." + name + ".bin")
    subprocess.check_call([str(H5DUMP), "-d", "/" + name, "-b", "LE", "-o", str(out), str(path)], stdout=subprocess.DEVNULL)
    return np.fromfile(out, dtype=dtype)


@pytest.mark.parametrize("method", ["nw", "sw"])
def test_cli_alignments(method, tmp_path, sa):
    from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
    from tests.test_neighbors_host import h5_dataset, h5_names
    n, k = 400, 5
    seqs = make_protein_set(n, 30, 150, 19)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, seqs)
    flags = ["-a", method, "-m", "blosum62", "-F"] + (["-p", 4] if method == "nw" else ["-s", 10, "-e", 1])
    for name, extra in (("full", []), ("only", ["--neighbors-only"])):
        out = tmp_path / f"{name}.h5"
        res = run("-i", fasta, "-o", out, *flags, "-k", k, "--alignments", *extra, "-B")
        assert "alignments of the 2000 neighbor pairs on the device" in res.stdout, res.stdout
        base = {"/sequences", "/neighbor_indices", "/neighbor_scores"} | (set() if extra else {"/similarity_matrix"})
        assert h5_names(out) == base | {"/neighbor_alignment_records", "/neighbor_cigar_offsets", "/neighbor_cigars"}
        index = h5_dataset(out, "neighbor_indices", (n, k))
        scores = h5_dataset(out, "neighbor_scores", (n, k))
        records = h5_typed(out, "neighbor_alignment_records", "<i4").reshape(n, k, 8)
        offsets = h5_typed(out, "neighbor_cigar_offsets", "<i8")
        cigars = h5_typed(out, "neighbor_cigars", "<u4")
        pairs = np.stack([np.repeat(np.arange(n), k), index.reshape(-1)], axis=1)
        want = sa.hip_alignments(store, scoring, pairs)
        flat = records.reshape(n * k, 8)
        for col, field in enumerate(FIELDS + ("cigar_len",)):
            assert np.array_equal(flat[:, col], want.records[field]), field
        assert np.array_equal(records[:, :, 0], scores)
        assert offsets.shape == (n * k + 1,) and np.array_equal(offsets[:-1], want.records["cigar_off"]) and offsets[-1] == len(cigars)
        assert np.array_equal(cigars, want.cigar)
    res = run("-i", fasta, "-o", tmp_path / "bad.h5", *flags, "--alignments", check=False)
    assert res.returncode == 1 and "--alignments requires -k" in res.stderr and not (tmp_path / "bad.h5").exists()
