#!/usr/bin/env python3
"""bench.py -- all-vs-all alignment throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 8            (spawns torch.distributed.run itself, one rank per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is ONE pass of the hot path over the whole workload, inputs resident in HBM, results delivered to host
memory -- the phase the reference's metric divides by (`pairs / alignment-phase seconds`, util/benchmark.c:63; the
phase brackets the launch/copy loop INCLUDING the device->host copies, interface/seqalign_cuda.c:182,292):
  N = 1   sa_ctx_align_host: every pair i<j scored (NW/BLOSUM62/gap 4 for the headline config) and the packed
          upper-triangular s32 vector copied into a page-locked host matrix, copies overlapping the kernels.
  N > 1   strong scaling (total work fixed): the launch plan's workgroup-tiles are dealt over the N ranks by DP work
          (sa_ctx_align_share); every rank's kernels store its scores densely for the exchange AND straight into ONE
          page-locked packed host matrix that all ranks attach (a shared mapping under /dev/shm) -- the device->host
          delivery of the reference's loop, without a copy pass; RCCL all-gathers over xGMI move the dense shares and
          sa_ctx_place_shares assembles the packed s32 matrix on every GPU -- all inside the timed step
          (sequencealigner_amd/distributed.py: TiledGatherStep).  After the timed steps every rank verifies windows of
          the gathered matrix and its slice of the host matrix, and rank 0 checks the assembled host matrix against the
          reference's per-column digests (tests/golden/digest_cfg2.npz).

A plain run sets up, warms up, times the --steps steps, writes the last step's result when --dump-outputs DIR is given
(DIR/scores.npy, DIR/scores_index.npy, DIR/scores_column_sums.npy: see dump_outputs) and prints the JSON line: metric,
value, unit, higher_is_better, dtype, ms_per_step, gcups and the workload.  Everything else below is measured and
checked only with --full (the --no-* switches trim that run):

Printed JSON (rank 0): metric/value per the driver contract, plus, with --full,
  device_resident -- the same pass with the result left in HBM (kernels only; >= value)
  host_boundary   -- sa_hip_align cold call (encode + upload + loop) and the `seqalign` CLI FASTA->HDF5 with -B
  roofline        -- dominant kernel vs the HBM roof, live HIP-event timing on the launch stream
  cpu_baseline    -- the reference's own CPU path (oracle/_ref, kind "reference") or our C restatement
                     (oracle/, kind "port") timed on this host's cores: the whole workload when that is projected to
                     take <= --cpu-full-seconds, else a bounded sample
  parity          -- the CPU scores of that leg compared, untimed, with the same prefix of the host-delivered matrix
  gcups, valu     -- the bound that actually constrains this integer DP
  extra.configs   -- cfg3 (Gotoh, full size) and the cfg4 shape (SW nuc44, one GPU's worth) measured the same way
  N > 1 also: the re-scored windows and host matrix checked on every rank, rank 0's reference-digest check
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import re
import socket
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9  # 256 CU x 4 SIMD-32 x 2.4 GHz = 7.86e13 s32 lane-ops/s
OPS_PER_CELL = {"nw": 5, "ga": 9, "sw": 11}  # reference op counts (nw.c:29-35, ga.c:47-62, sw.c:39-57)
# SIMD issue cycles one wave64 DP cell costs at the very least with the packed-u16 formulation of the 8-lane classes
# (three-way maxima are one v_pk_maximum3_f16): per TWO cells NW = 1 plain 32-bit add + 1 VOP3P,
# Gotoh = 2 + 3, SW = 3 + 3.5.  Instruction costs measured on this chip with long kernels against the wall clock
# (profiles/r02_microbench_nw_chain_dependency_shapes.txt, r02_microbench_valu_rates_wallclock.txt,
# r02i_microbench_max3_f16.txt): VOP3 / VOP3P / SDWA / DPP ~4.1 SIMD cycles per wave64 instruction, plain 32-bit VOP2
# ~2.5 -- the guide's "2 cycles" row is the plain-VOP2 / v_fma_f32 class.
CYC_SLOW, CYC_FAST = 4.1, 2.5
MIN_ISSUE_CYCLES_PER_CELL = {"nw": (1 * CYC_FAST + 1 * CYC_SLOW) / 2, "ga": (2 * CYC_FAST + 3 * CYC_SLOW) / 2,
                             "sw": (3 * CYC_FAST + 3.5 * CYC_SLOW) / 2}
SIMDS, SHADER_HZ = 256 * 4, 2.4e9
CFG4_SHAPE_N = 12_000  # "cfg4 shape": the cfg4 generator and scoring at a size one GPU finishes in a fraction of a second


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--n", "--nseq", dest="n", type=int, default=None, help="override sequence count (parity/debug runs)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: device-resident pass, roofline, host boundary, "
                         "CPU baseline and parity, extra configs (N > 1: per-rank verification, digests, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's result matrix (a fixed sample of it) to DIR/*.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU-baseline duration of a bounded sample")
    ap.add_argument("--cpu-full-seconds", type=float, default=100.0,
                    help="run the CPU reference over the WHOLE workload (and compare every score) when that is projected to take at most this long")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-boundary", action="store_true", help="skip the sa_hip_align / CLI end-to-end legs (profiling runs)")
    ap.add_argument("--no-extra", action="store_true", help="skip the extra.configs legs (cfg3, cfg4 shape)")
    ap.add_argument("--device-resident-only", action="store_true", help="time the kernels only (result stays in HBM): profiling runs")
    ap.add_argument("--chunks", type=int, default=None, help="super-chunks per step for compute/all-gather overlap (N>1; default: pick 1, 2 or 4 by an untimed trial)")
    return ap.parse_args()


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start one rank per GPU with torch.distributed.run as a CHILD
    process (nothing in this process has touched the GPU) and relay its output and exit code."""
    import torch
    have = torch.cuda.device_count()  # does not initialise the runtime on this image
    if have < args.gpus:
        print(f"bench.py: --gpus {args.gpus} needs {args.gpus} visible GPUs, this box has {have}; "
              f"one rank per GPU over RCCL cannot be started (run with --gpus {max(have, 1)})", file=sys.stderr, flush=True)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(ROOT / "bench.py"), *sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


ARITH = ("packed kernels: two DP cells per 32-bit lane as u16 halves (v_pk_maximum3_f16 / v_pk_max_u16 + plain 32-bit adds), "
         "entered only under the host's range predicate for the scoring and column class (DESIGN.md 4.2, csrc/sa_limits.cpp) and "
         "bit-exact with the reference's s32 arithmetic; everything else runs the s32 kernels -- results are s32 either way")
_cpu_scores = {}  # workload key -> (n, scores) of the CPU reference run, for legs that time other kernels on the same input


def cpu_baseline(seqs, cfg, target_s: float, full_s: float, got=None, key=None) -> tuple[dict, dict | None]:
    """Reference CPU path on the same workload (pairs/s, all host cores) -> (cpu_baseline, parity).

    A calibration run on 600 sequences projects the whole workload; when the projection is within `full_s` seconds the
    reference runs over the WHOLE workload -- that run is then the baseline measurement -- otherwise over a prefix
    sized for `target_s` seconds.  Either way the scores it returns are compared, untimed, with the same prefix of the
    host-delivered matrix `got` (the packed index of the first n sequences is the first n(n-1)/2 elements): `parity`."""
    import numpy as np
    import sequencealigner_amd as sa
    from tests.oracle_binding import Oracle, RefLib, ref_available

    ncores = os.cpu_count() or 1
    oracle = Oracle()
    threads = min(ncores, oracle.max_threads)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])

    def run(n, use_ref):
        store = sa.SequenceStore.from_sequences(seqs[:n])
        if use_ref:
            ref = RefLib(cfg["method"], cfg["matrix"], threads=threads, **cfg["gaps"])
            try:
                t = time.perf_counter()
                scores = ref.align(store, triangular=True)
                return time.perf_counter() - t, store, scores
            finally:
                ref.close()
        t = time.perf_counter()
        scores = oracle.align(store, scoring, triangular=True, threads=threads)
        return time.perf_counter() - t, store, scores

    use_ref = False
    if ref_available():
        try:
            run(64, True)
            use_ref = True
        except Exception:
            use_ref = False
    n0 = min(len(seqs), 600)
    t0, _, _ = run(n0, use_ref)
    rate = (n0 * (n0 - 1) / 2) / max(t0, 1e-6)
    total_pairs = len(seqs) * (len(seqs) - 1) / 2
    full = total_pairs / rate <= full_s
    n = len(seqs) if full else int(min(len(seqs), max(n0, (2 * rate * target_s) ** 0.5)))
    t, store, scores = run(n, use_ref)
    pairs = n * (n - 1) // 2
    base = {
        "value": pairs / t, "unit": "pair-alignments/s", "cores": threads,
        "kind": "reference" if use_ref else "port",
        "sample": (f"the whole workload: {n} sequences = {pairs} pairs, {store.cells()} cells, {t:.2f} s" if full else
                   f"first {n} sequences of the workload = {pairs} pairs, {store.cells()} cells, {t:.2f} s"),
        "gcups": store.cells() / t / 1e9,
    }
    parity = None
    if key is not None:
        _cpu_scores[key] = (n, scores, "reference" if use_ref else "port", bool(full))
    if got is not None:
        mism = int(np.count_nonzero(np.asarray(got[:pairs]) != scores))
        parity = {"pairs_compared": pairs, "mismatches": mism, "against": "reference" if use_ref else "port",
                  "whole_workload": bool(full), "compared": "host-delivered packed matrix (sa_ctx_align_host, the timed path) vs the CPU scores"}
    return base, parity


def roofline_of(tm: dict, store, steps: int, workload: str, world: int, full_size: bool = True) -> dict:
    """dominant kernel: algorithmic HBM bytes of ONE launch (4 B per pair written + the sequence store
    and its offsets read once) / that kernel's average launch duration (HIP events on the launch stream)"""
    launches = max(tm["launches"], 1)
    k_pairs = tm["pairs"] // launches
    alg_bytes = 4 * k_pairs + int(store.blob.size) + 8 * store.num
    avg_ms = tm["ms"] / launches
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    # HBM traffic of that kernel per launch from the committed PMC passes (profiles/*_traffic.json), if the workload,
    # launch size and kernel match; null otherwise (it cannot be measured inside this process)
    traffic = None
    for tf in sorted((ROOT / "profiles").glob("*_traffic.json")):
        tj = json.loads(tf.read_text())
        # (a file that does not say which launch it measured -- sequence count and pairs per launch -- is never quoted)
        if (tj.get("kernel") == tm["kernel"] and tj.get("workload") == workload and world == 1
                and tj.get("n_sequences") == store.num and "pairs_per_launch" in tj
                and abs(tj["pairs_per_launch"] - k_pairs) <= 0.02 * k_pairs):
            traffic = tj["traffic_bytes_per_launch"]
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "kernel": tm["kernel"], "kernel_avg_ms": avg_ms, "launches": tm["launches"],
            "algorithmic_bytes_per_launch": alg_bytes, "pairs_per_launch": k_pairs,
            "sum_of_kernel_ms_per_step": tm["all_kernels_ms"] / steps,
            "note": "per-class kernels of one range overlap on side streams; durations are per launch as rocprofv3 reports them"}


def valu_of(method: str, cells: int, seconds: float) -> dict:
    gcups = cells / seconds / 1e9
    return {"gcups_this_rank": gcups, "reference_ops_per_cell": OPS_PER_CELL[method],
            "min_issue_cycles_per_wave_cell": MIN_ISSUE_CYCLES_PER_CELL[method],
            "cycles_per_wave64_inst": {"vop3_vop3p_sdwa_dpp": CYC_SLOW, "plain_vop2": CYC_FAST},
            # wave-cells x minimal issue cycles per cell / SIMD cycles available in the step (1024 SIMDs at 2.4 GHz)
            "frac_of_valu_issue_bound": (cells / 64) * MIN_ISSUE_CYCLES_PER_CELL[method] / (seconds * SIMDS * SHADER_HZ)}


def time_host_steps(ctx, dest, steps: int, warmup: int, torch) -> tuple[float, dict]:
    """steps x sa_ctx_align_host (launch + device->host copy loop into the page-locked packed matrix)"""
    for _ in range(warmup):
        ctx.align_host(dest.array, triangular=True)
    torch.cuda.synchronize()
    ctx.timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.align_host(dest.array, triangular=True)  # returns when the last copy has landed
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    tm = ctx.timing_read()
    ctx.timing(False)
    return elapsed, tm


def time_resident_steps(ctx, packed, pairs: int, steps: int, warmup: int, torch) -> tuple[float, dict]:
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        ctx.align_range(0, pairs, packed.data_ptr(), s)
    torch.cuda.synchronize()
    ctx.timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.align_range(0, pairs, packed.data_ptr(), s)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    tm = ctx.timing_read()
    ctx.timing(False)
    return elapsed, tm


def cli_leg(seqs, cfg, quiet: bool = True, extra_flags=(), keep_size: bool = False) -> dict | None:
    """The product as a user runs it: `cli/seqalign -i x.fasta -o x.h5 ... -B` from a cold process."""
    exe = ROOT / "cli" / "seqalign"
    if not exe.exists():
        return None
    with tempfile.TemporaryDirectory(prefix="sa_bench_") as tmp:
        fasta = pathlib.Path(tmp) / "in.fasta"
        with open(fasta, "wb") as f:
            for k, s in enumerate(seqs):
                f.write(b">s%d\n" % k + s + b"\n")
        g = cfg["gaps"]
        gaps = ["-p", str(g["gap_pen"])] if "gap_pen" in g else ["-s", str(g["gap_open"]), "-e", str(g["gap_extend"])]
        cmd = [str(exe), "-i", str(fasta), "-o", str(pathlib.Path(tmp) / "out.h5"), "-a", cfg["method"], "-m", cfg["matrix"], *gaps,
               *map(str, extra_flags), "-B", "-F", *(["-Q"] if quiet else [])]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t0
        out_h5 = pathlib.Path(tmp) / "out.h5"
        file_bytes = out_h5.stat().st_size if keep_size and out_h5.exists() else None
    txt = r.stdout + r.stderr
    if r.returncode != 0:
        return {"error": txt[-400:], "returncode": r.returncode}

    def grab(label):
        m = re.search(label + r":\s*([0-9.]+)", txt)
        return float(m.group(1)) if m else None
    return {"command": " ".join(["cli/seqalign", *cmd[1:2], "in.fasta", "-o", "out.h5", *cmd[5:]]),
            "alignments_per_second": grab("Alignments per second"), "input_s": grab("Input"), "filter_s": grab("Filter"),
            "alignment_s": grab("Alignment"), "output_s": grab("Output"), "setup_s": grab(r"outside the phases as in the reference"),
            "process_wall_s": wall, **({"file_bytes": file_bytes} if keep_size else {}),
            "note": "cold process, FASTA -> full N x N HDF5, the chunks tiled on the device and written while the next column blocks are "
                    "aligned (DESIGN.md 4.8); alignment = the device's alignment time (reference's bench_align bracket), output = the "
                    "rest of that section, setup = context, code-object load, upload, buffers (outside the phases as in the reference)"}


def extra_config(name: str, n, steps: int, cpu_seconds: float, cpu_full_seconds: float, torch, sa, make_config) -> dict:
    """cfg3 / cfg4-shape leg: the same measurement as the headline, a few steps, in this process"""
    seqs, cfg = make_config(name, n)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    pairs, cells = store.pairs, store.cells()
    ctx = sa.Context(store, scoring, 0)
    dest = sa.PinnedMatrix(pairs)
    base = parity = None
    try:
        elapsed, tm = time_host_steps(ctx, dest, steps, 1, torch)
        packed = torch.empty(pairs, dtype=torch.int32, device="cuda")
        el_res, _ = time_resident_steps(ctx, packed, pairs, steps, 1, torch)
        same = bool((torch.from_numpy(dest.array).cuda() == packed).all().item())
        del packed
        ctx.close()
        if cpu_seconds > 0:
            base, parity = cpu_baseline(seqs, cfg, cpu_seconds, cpu_full_seconds, dest.array)
    finally:
        ctx.close()
        dest.close()
    sec = elapsed / steps
    out = {"workload": f"{name}{'' if n is None else ' shape'}: {store.num} {cfg['kind']} seqs x U[{cfg['lo']},{cfg['hi']}], {cfg['method']} {cfg['matrix']} {cfg['gaps']}",
           "pairs": pairs, "cells": cells, "steps": steps, "ms_per_step": sec * 1e3, "value": pairs / sec, "unit": "pair-alignments/s",
           "gcups": cells / sec / 1e9,
           "device_resident": {"ms_per_step": el_res / steps * 1e3, "value": pairs * steps / el_res, "gcups": cells * steps / el_res / 1e9},
           "host_result_equals_device_result": same,
           "roofline": roofline_of(tm, store, steps, name, 1, n is None), "valu": valu_of(cfg["method"], cells, sec)}
    out["cpu_baseline"] = base
    out["parity"] = parity
    return out


def s32_kernels_leg(seqs, cfg, steps: int, torch, sa) -> dict:
    """the headline workload on the s32 systolic kernels (SA_HIP_NO_PK=1: no packed-u16 classes), host-delivered, with its
    own parity block against the CPU scores of the headline leg"""
    import numpy as np
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    os.environ["SA_HIP_NO_PK"] = "1"  # (read when the context is created)
    try:
        ctx = sa.Context(store, scoring, 0)
    finally:
        del os.environ["SA_HIP_NO_PK"]
    dest = sa.PinnedMatrix(store.pairs)
    try:
        elapsed, tm = time_host_steps(ctx, dest, steps, 1, torch)
        sec = elapsed / steps
        out = {"switch": "SA_HIP_NO_PK=1", "dtype": "s32", "steps": steps, "ms_per_step": sec * 1e3, "value": store.pairs / sec,
               "unit": "pair-alignments/s", "gcups": store.cells() / sec / 1e9, "dominant_kernel": tm["kernel"], "parity": None}
        if "cfg2" in _cpu_scores:
            n, scores, against, whole = _cpu_scores["cfg2"]
            k = n * (n - 1) // 2
            out["parity"] = {"pairs_compared": k, "mismatches": int(np.count_nonzero(dest.array[:k] != scores)), "against": against,
                             "whole_workload": whole, "compared": "host-delivered matrix of the s32 kernels vs the CPU scores of the headline leg"}
        return out
    finally:
        ctx.close()
        dest.close()


def deflate_leg(seqs, cfg, torch, sa) -> dict:
    """the `-z` path of the tool on the headline workload: the N x N matrix as HDF5 chunks (4096 x 4096), deflated on the device
    (csrc/sa_deflate.hip).  Every tile is inflated with stock zlib and compared with the matrix the CPU scores give (the
    reference's own when the headline leg ran it), zero diagonal and zero padding included."""
    import zlib
    import numpy as np
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    n, chunk = store.num, 4096
    d = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
    with sa.Context(store, scoring, 0) as ctx:
        ctx.align_range(0, store.pairs, d.data_ptr())
        torch.cuda.synchronize()
    against = "device scores"
    tri = None
    if "cfg2" in _cpu_scores and _cpu_scores["cfg2"][0] == n:
        tri, against = _cpu_scores["cfg2"][1], _cpu_scores["cfg2"][2]
    if tri is None:
        tri = d.cpu().numpy()
    out = {"chunk": chunk, "level": "fixed parse + dynamic Huffman (DESIGN.md 4.8)"}
    for trial in range(2):  # (the second walk is the timed one: buffers page-locked, code objects loaded)
        with sa.DeflateJob(n, chunk, d_packed_ptr=d.data_ptr()) as job:
            t0 = time.perf_counter()
            rows = [job.tile_row(r) for r in range(job.tiles_per_row)]
            wall = time.perf_counter() - t0
            st = job.stats()
    nc = len(rows)
    mism = tiles = 0
    jj = np.repeat(np.arange(n), np.arange(n))
    ii = np.concatenate([np.arange(k) for k in range(n)])
    full = np.zeros((nc * chunk, nc * chunk), np.int32)
    full[ii, jj] = tri
    full[jj, ii] = tri
    for r in range(nc):
        for c in range(nc):
            got = np.frombuffer(zlib.decompress(rows[r][c]), "<i4").reshape(chunk, chunk)
            mism += int(np.count_nonzero(got != full[r * chunk:(r + 1) * chunk, c * chunk:(c + 1) * chunk]))
            tiles += 1
    out.update({"raw_bytes": st["raw_bytes"], "stream_bytes": st["out_bytes"], "ratio": st["raw_bytes"] / st["out_bytes"],
                "walk_seconds": wall, "matrix_gb_per_s": st["raw_bytes"] / wall / 1e9,
                "note": "walk = encode + gather + device->host copy + the binding's copy of every stream into Python bytes; the kernels "
                        "alone: profiles/r04d_deflate_encoder_summary.txt",
                "parity": {"tiles_inflated": tiles, "elements_compared": tiles * chunk * chunk, "mismatches": mism, "against": against,
                           "compared": "zlib.decompress of every tile vs the full symmetric matrix of the CPU scores (zero diagonal, zero padding)"}})
    return out


def tool_end_to_end_leg(make_config) -> dict:
    """BASELINE configs 5 and 4 END TO END through the product, at their full size on this one device: cli/seqalign from a cold
    process, FASTA -> N x N HDF5 (config 5 with its options -f 0.9 -z 6: device filter, alignment in column blocks, the tiles of
    every shell deflated on the device and written meanwhile; config 4 without -z: raw tiles).  Needs ~25 GB of scratch space
    for the two 11 GB files (one at a time); skipped without it.  Parity of exactly this path at exactly this size:
    tests/test_gpu_stripes.py::test_full_size_tool_output_matches_the_reference."""
    import shutil
    free = shutil.disk_usage(tempfile.gettempdir()).free
    if free < 30 * 2**30:
        return {"skipped": f"{free / 2**30:.0f} GB free under {tempfile.gettempdir()}: needs 30"}
    out = {}
    for name, flags in (("cfg5", ["-f", "0.9", "-z", "6"]), ("cfg4", [])):
        seqs, cfg = make_config(name)
        leg = cli_leg(seqs, cfg, quiet=True, extra_flags=flags, keep_size=True) or {"error": "cli/seqalign is not built"}
        leg["sequences_in"] = len(seqs)
        leg.pop("note", None)
        if "error" not in leg:
            leg["total_s"] = sum(leg.get(k) or 0.0 for k in ("input_s", "filter_s", "alignment_s", "output_s"))
        out[name] = leg
    out["note"] = ("total_s = the tool's own phases (input + filter + alignment + output; alignment and output overlap: output is what the "
                   "output section took beyond the device's alignment time); process_wall_s adds loading, device set-up and exit. "
                   "History of config 5's total: zlib -6 on every core 159.8 s (profiles/r04_cli_cfg5_full_size_end_to_end.txt)")
    return out


DUMP_SAMPLE = 2_000_000  # scores written by --dump-outputs at most: with their indices 32 MB of float64
DUMP_SEED = 20_240_601


def dump_outputs(path: str, scores, num: int) -> None:
    """--dump-outputs: the packed upper-triangular s32 score vector of the last timed step (what the caller of the timed
    path receives), as float64 (exact for every s32).  scores.npy holds the elements at scores_index.npy: all of them
    when that fits, else a fixed seeded uniform sample (sorted); scores_column_sums.npy sums every column j (the scores of
    pairs (i, j), i < j, j >= 1) so that no element goes unchecked.  The same arguments give the same input and the same
    indices on every run."""
    import numpy as np
    out = pathlib.Path(path)
    out.mkdir(parents=True, exist_ok=True)
    scores = np.asarray(scores)
    total = scores.size
    if total <= DUMP_SAMPLE:
        idx = np.arange(total, dtype=np.int64)
    else:
        idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, total, DUMP_SAMPLE, dtype=np.int64))
    np.save(out / "scores.npy", scores[idx].astype(np.float64))
    np.save(out / "scores_index.npy", idx.astype(np.float64))
    starts = np.arange(1, num, dtype=np.int64) * np.arange(0, num - 1, dtype=np.int64) // 2  # first element of column j = j(j-1)/2
    sums = np.add.reduceat(scores, starts, dtype=np.int64) if num > 1 else np.zeros(0, np.int64)
    np.save(out / "scores_column_sums.npy", sums.astype(np.float64))


_json_fd = None


def emit(line: dict) -> None:
    """the ONE JSON line of the run, on the process's original stdout"""
    data = (json.dumps(line) + "\n").encode()
    if _json_fd is None:
        sys.stdout.write(data.decode())
        sys.stdout.flush()
    else:
        os.write(_json_fd, data)


def main():
    global _json_fd
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1 and not os.environ.get("SA_BENCH_FORCE_DIST"):
        raise SystemExit(self_launch(args))
    # stdout carries the JSON line and nothing else: whatever libraries print there (RCCL announces its version on stdout
    # when a communicator comes up) goes to stderr instead
    sys.stdout.flush()
    _json_fd = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch
    import sequencealigner_amd as sa
    from sequencealigner_amd.distributed import GatherStep, HipShares, TiledGatherStep
    from tests.synth import CONFIGS, make_config

    if args.config not in CONFIGS:
        raise SystemExit(f"unknown --config {args.config}; one of {sorted(CONFIGS)}")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        args.gpus = world
    # SA_BENCH_ONE_GPU_REHEARSAL=1 (development): every rank on device 0 and the collective over gloo, staged through
    # the host -- RCCL refuses two ranks on one device.  Rehearses THIS file's N > 1 code with world >= 2 on a one-GPU box
    # (shared host matrix, trial, all-gather, verification); its timings mean nothing.
    rehearsal = bool(os.environ.get("SA_BENCH_ONE_GPU_REHEARSAL"))
    rdev = "cpu" if rehearsal else "cuda"  # where the small reduction tensors live
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or os.environ.get("SA_BENCH_FORCE_DIST"):  # the env switch rehearses the RCCL path on one GPU
        import torch.distributed as dist
        if "MASTER_ADDR" not in os.environ:  # 1-rank rehearsal without a launcher
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29517"), RANK="0", WORLD_SIZE="1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    seqs, cfg = make_config(args.config, args.n)
    store = sa.SequenceStore.from_sequences(seqs)
    scoring = sa.Scoring.from_names(cfg["method"], cfg["matrix"], **cfg["gaps"])
    method = scoring.method_name
    pairs = store.pairs
    cells = store.cells()
    use_dist = dist is not None
    ctx = sa.Context(store, scoring, local_rank)
    out = None

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    workload = (f"{args.config}: {store.num} {cfg['kind']} seqs x U[{cfg['lo']},{cfg['hi']}], "
                f"{cfg['method']} {cfg['matrix']} {cfg['gaps']}, all-vs-all packed triangular")
    if not use_dist:
        # ---- N = 1: the reference's phase = launch + device->host copy loop, page-locked destination ----
        # (the device-resident pass runs first, as its own warmed-up timing, only with --full or when it is the headline)
        packed = None
        if args.full or args.device_resident_only:
            packed = torch.empty(pairs, dtype=torch.int32, device="cuda")
            el_res, tm_res = time_resident_steps(ctx, packed, pairs, args.steps, args.warmup, torch)
        if args.device_resident_only:
            elapsed, tm, dest = el_res, tm_res, None
        else:
            dest = sa.PinnedMatrix(pairs)
            elapsed, tm = time_host_steps(ctx, dest, args.steps, args.warmup, torch)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, dest.array if dest is not None else packed.cpu().numpy(), store.num)
        sec = elapsed / args.steps
        out = {
            "metric": "pair-alignments/sec", "value": pairs / sec, "unit": "pair-alignments/s",
            "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": sec * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u16x2", "arith": ARITH, "data": "synthetic",
            "config": {"workload": workload, "pairs": pairs, "cells": cells, "parallelism": "pair-range x1",
                       "timed_region": ("kernels only, result left in HBM (--device-resident-only)" if args.device_resident_only else
                                        "sa_ctx_align_host: launch + device->host copy loop into a page-locked packed host matrix "
                                        "(the reference's bench_align bracket, seqalign_cuda.c:182,292); inputs resident in HBM")},
            "gcups": cells / sec / 1e9,
            "device": sa.device_name(local_rank),
        }
        if not args.full:
            ctx.close()
            if dest is not None:
                dest.close()
            emit(out)
            return
        if dest is not None:
            assert np.array_equal(dest.array, packed.cpu().numpy()), "host-delivered result differs from device-resident result"
        out.update({
            "device_resident": {"value": pairs * args.steps / el_res, "ms_per_step": el_res / args.steps * 1e3,
                                "gcups": cells * args.steps / el_res / 1e9,
                                "note": "same pass, result left in HBM (kernels only); round-1 headline definition"},
            "roofline": roofline_of(tm, store, args.steps, args.config, 1, args.n is None),
            "valu": valu_of(method, cells, sec),
        })
        if not args.no_host_boundary:
            t1 = time.perf_counter()
            host = sa.hip_align(store, scoring, triangular=True)
            e2e = time.perf_counter() - t1
            e2e_phase = sa.last_align_seconds()
            assert np.array_equal(host, packed.cpu().numpy()), "host-boundary result differs from device-resident result"
            del host
            out["host_boundary"] = {
                "seconds": e2e, "pairs_per_s": pairs / e2e, "align_phase_seconds": e2e_phase,
                # the cold call itemised by the library (sa_hip_last_align_breakdown): everything but phase_ms is set-up
                # the reference keeps outside its bracket too; matrix_alloc_ms = the binding's zero-filled numpy matrix
                **sa.last_align_breakdown(), "matrix_alloc_and_call_overhead_ms": e2e * 1e3 - sa.last_align_breakdown().get("total_ms", 0.0),
                "align_phase_pairs_per_s": pairs / e2e_phase if e2e_phase > 0 else None,
                "note": "one sa_hip_align call on a pageable destination: encode + context + upload + page-locking + loop; "
                        "align_phase = its launch/copy loop only",
                "cli": cli_leg(seqs, cfg),
                # ... and as a user starts it, progress line and all (no -Q): the listener must not cost the phase anything
                "cli_default_verbosity": {k: v for k, v in (cli_leg(seqs, cfg, quiet=False) or {}).items()
                                          if k in ("alignment_s", "alignments_per_second", "process_wall_s", "error", "returncode")}}
        del packed
        ctx.close()
        if not args.no_cpu_baseline:
            out["cpu_baseline"], out["parity"] = cpu_baseline(seqs, cfg, args.cpu_seconds, args.cpu_full_seconds,
                                                              dest.array if dest is not None else None, key=args.config)
        if dest is not None:
            dest.close()
        if not args.no_extra and args.config == "cfg2" and args.n is None and not args.device_resident_only:
            cpu_s = 0.0 if args.no_cpu_baseline else max(3.0, args.cpu_seconds / 2)
            extra = {}
            for key, (name, n) in {"cfg3": ("cfg3", None), "cfg4": ("cfg4", CFG4_SHAPE_N)}.items():
                extra[key] = extra_config(name, n, 3, cpu_s, args.cpu_full_seconds, torch, sa, make_config)
            # the length distribution the headline does not show: 8000 x U[20,190] (171 distinct lengths: few equal lengths per
            # arranged block, so most rounds of a tile are mixed -- DESIGN.md 4.2)
            extra["mixed"] = extra_config("mixed", None, 3, cpu_s, args.cpu_full_seconds, torch, sa, make_config)
            out["extra"] = {"configs": extra,
                            # the same cfg 2 step with the packed kernels switched off: the reference-width (s32) systolic kernels
                            "s32_kernels": s32_kernels_leg(seqs, cfg, 3, torch, sa),
                            # the -z path: the matrix as HDF5 chunks deflated on the device, every tile inflated and compared
                            "deflate": deflate_leg(seqs, cfg, torch, sa),
                            # BASELINE configs 5 and 4 end to end through the tool at full size (one device)
                            "tool_end_to_end": tool_end_to_end_leg(make_config)}
        emit(out)
        return

    # ---- N > 1 (or the 1-rank RCCL rehearsal): tile-interleaved shares + overlapped all-gathers + per-rank host delivery ----
    # exchange format of the all-gather: int16 when every score of this workload provably fits (half the bytes over
    # xGMI); the gathered shares are widened to the reference's s32 and placed into packed order on every GPU inside
    # the timed step
    use16 = ctx.scores_fit16 and not os.environ.get("SA_BENCH_GATHER32")
    # partition of the pair space over the ranks: "tiled" (the launch plan's tiles dealt by DP work, dense shares, widen-and-
    # place, kernels deliver to the host matrix) or "range" (contiguous packed ranges, in-place gather, every rank copies
    # 1/N).  SA_BENCH_PARTITION fixes it; otherwise both are tried, untimed, next to the super-chunk counts.
    forced = os.environ.get("SA_BENCH_PARTITION")
    partitions = [forced] if forced in ("tiled", "range") else ["tiled", "range"]

    # the host matrix of the tiled step: ONE packed matrix for the node, a shared mapping under /dev/shm that every rank
    # attaches and page-locks (the reference's single mmap-ed result, io/output.c:55); every rank's kernels store the
    # scores that rank computed straight into it, so together the ranks fill it exactly once
    cpu_flag = pathlib.Path(f"/dev/shm/sa_bench_cpu_done_{os.environ.get('MASTER_PORT', '0')}_{os.getuid()}")
    if rank == 0:
        cpu_flag.unlink(missing_ok=True)  # (left behind by a run that died between its CPU leg and its last barrier)
    fence()
    host = None
    if "tiled" in partitions:
        shm = f"/dev/shm/sa_bench_matrix_{os.environ.get('MASTER_PORT', '0')}_{os.getuid()}.bin"
        if rank == 0:
            host = sa.PinnedMatrix(pairs, shared=shm, create=True)
        fence()
        if rank != 0:
            host = sa.PinnedMatrix(pairs, shared=shm, create=False)
        fence()

    class _GlooViaHost:  # (rehearsal only: gloo moves host tensors)
        @staticmethod
        def all_gather_into_tensor(out, inp):
            o = torch.empty(out.shape, dtype=out.dtype)
            dist.all_gather_into_tensor(o, inp.cpu())
            out.copy_(o)

    def make_step(part, c):
        if part == "tiled":
            return TiledGatherStep(HipShares(ctx, use16, host), store.num, world, rank, c, _GlooViaHost if rehearsal else dist)
        return GatherStep(ctx, pairs, world, rank, c, _GlooViaHost if rehearsal else dist, use16)

    # super-chunks per step: more of them hide more of the all-gather / place / host copy behind the kernels but add
    # launches; the trade depends on the fabric, so (unless --chunks fixes it) it is measured before the warmup,
    # untimed, and every rank takes the same decision from the max-over-ranks time
    candidates = [(part, c) for part in partitions for c in ([args.chunks] if args.chunks else ([1, 2, 3] if part == "tiled" else [1, 2]))]
    tuned = {}
    if len(candidates) > 1:
        for part, c in candidates:
            trial = make_step(part, c)
            trial(); trial()
            fence()
            t0 = time.perf_counter()
            for _ in range(4):
                trial()
            fence()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=rdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            tuned[f"{part} x{c}"] = float(t.item()) / 4 * 1e3
            del trial
            torch.cuda.empty_cache()
        best = min(tuned, key=tuned.get)
        tiled_best = min((k for k in tuned if k.startswith("tiled")), key=tuned.get, default=None)
        if tiled_best is not None and tuned[tiled_best] <= 1.02 * tuned[best]:
            best = tiled_best  # (within the noise of a 4-step trial: the schedule whose host matrix the reference digests check)
        candidates = [c for c in candidates if f"{c[0]} x{c[1]}" == best]
    tiled = candidates[0][0] == "tiled"
    step = make_step(*candidates[0])
    nchunks = step.chunks if tiled else step.sched.chunks
    my_cells = cells // world  # (tiled: the ranks' shares are balanced by DP work)
    if not tiled:
        my_cells = sum(store.cells(lo, hi - lo) for lo, hi in (step.sched.slice_range(c) for c in range(nchunks)))

    for _ in range(args.warmup):
        step()
    fence()
    ctx.timing(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    tm = ctx.timing_read()
    ctx.timing(False)
    t = torch.tensor([elapsed], dtype=torch.float64, device=rdev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, host.array if tiled else step.packed.cpu().numpy(), store.num)

    gather_ok = digest_ok = None
    if args.full:
        # every rank re-scores a few random windows of the gathered vector with its own kernels (untimed) and compares; the
        # host matrix -- filled by all ranks' direct stores during the last step -- must equal the gathered vector element
        # for element: rank r checks slice r of it.  (The oracle-backed check of this schedule: tests/test_gpu_gather_step.py,
        # the reference-digest check of placed shares and host matrix: tests/test_gpu_digests.py)
        vrng = np.random.default_rng(1234 + rank)
        okflag = 1
        for _ in range(6):
            w = int(min(pairs, 65536))
            a0 = int(vrng.integers(0, pairs - w + 1))
            chk = torch.empty(w, dtype=torch.int32, device="cuda")
            ctx.align_range(a0, w, chk.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if not torch.equal(chk, step.packed[a0:a0 + w]):
                okflag = 0
        fence()
        if tiled:
            per = (pairs + world - 1) // world
            lo, hi = min(pairs, rank * per), min(pairs, (rank + 1) * per)
            if not np.array_equal(host.array[lo:hi], step.packed[lo:hi].cpu().numpy()):
                okflag = 0
        else:
            for lo, hi, ho in step.host_ranges():
                if not torch.equal(step.host[ho:ho + hi - lo], step.packed[lo:hi].cpu()):
                    okflag = 0
        t = torch.tensor([okflag], dtype=torch.int32, device=rdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        gather_ok = bool(t.item())
        # rank 0: the assembled host matrix against the reference's per-column digests of this workload, when the build
        # container committed them (tests/golden/digest_<config>.npz) -- every pair, bit for bit, no sampling
        dpath = ROOT / "tests" / "golden" / f"digest_{args.config}.npz"
        if tiled and rank == 0 and args.n is None and dpath.exists():
            from tests.digest_util import column_digests
            z = np.load(dpath)
            got = column_digests(host.array, store.num)
            digest_ok = all(bool(np.array_equal(got[k], z[k])) for k in ("sum", "xor", "crc32"))

    # rank 0 alone times the reference's CPU path on a bounded sample of the workload (all host cores) and compares its
    # scores with the same prefix of the host matrix the ranks filled; the other ranks sleep on a flag file meanwhile
    base = parity = None
    flag = cpu_flag
    if rank == 0:
        try:
            if args.full and not args.no_cpu_baseline:
                result = host.array if tiled else step.packed.cpu().numpy()
                base, parity = cpu_baseline(seqs, cfg, args.cpu_seconds, 0.0, result)
                if parity is not None:
                    parity["compared"] = (("the ONE host matrix all ranks' kernels stored into" if tiled else "the gathered packed vector of rank 0")
                                          + " vs the CPU scores")
        finally:
            flag.touch()
    else:
        while not flag.exists():
            time.sleep(0.2)
    dist.barrier()
    if rank == 0:
        flag.unlink(missing_ok=True)
        sec = elapsed / args.steps
        out = {
            "metric": "pair-alignments/sec", "value": pairs / sec, "unit": "pair-alignments/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": sec * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u16x2", "arith": ARITH, "data": "synthetic",
            "config": {"workload": workload, "pairs": pairs, "cells": cells,
                       "parallelism": f"{'tiles of the launch plan dealt over' if tiled else 'contiguous pair ranges on'} {world} ranks + RCCL all-gather "
                                      f"({'int16 exchange, widened to s32 on device' if use16 else 's32'}), "
                                      f"{nchunks} overlapped super-chunks, " + ("every rank's kernels store its scores straight into the one page-locked host matrix (shared mapping)" if tiled else f"every rank copies its 1/{world} share to page-locked host memory"),
                       "timed_region": f"kernels (with host delivery) + all-gathers + widen-and-place ({'TiledGatherStep' if tiled else 'GatherStep'}); inputs resident in HBM",
                       **({"super_chunk_trial_ms": tuned} if tuned else {})},
            "gcups": cells / sec / 1e9,
            "device": sa.device_name(local_rank),
        }
        if args.full:
            out["config"].update({"gathered_and_host_result_verified_on_every_rank": gather_ok,
                                  "host_matrix_equals_reference_digests": digest_ok})
            out.update({"roofline": roofline_of(tm, store, args.steps, args.config, world, args.n is None),
                        "valu": valu_of(method, my_cells, sec), "cpu_baseline": base, "parity": parity})
        emit(out)
    ctx.close()
    dist.barrier()
    if host is not None:
        host.close()
        if rank == 0:
            try:
                os.unlink(host.path)
            except OSError:
                pass
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
