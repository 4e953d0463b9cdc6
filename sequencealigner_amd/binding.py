"""ctypes binding of include/seqalign_hip.h (no torch dependency; torch is only plumbing for callers)."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import pathlib
import sys
from dataclasses import dataclass, field
from typing import Iterable, Optional, Sequence

import numpy as np

_LIB_PATH = pathlib.Path(__file__).resolve().parent / "lib" / "libseqalign_hip.so"
_lib: Optional[C.CDLL] = None

LUT_SIZE = 128
NEIGHBORS_MAX = 64  # SA_HIP_NEIGHBORS_MAX
SUB_DIM = 24
SCORE_MIN = -(1 << 30)  # reference src/bio/align.h:19

METHOD_NW, METHOD_GA, METHOD_SW = 0, 1, 2
GAP_LINEAR, GAP_AFFINE = 0, 1


class AlignError(RuntimeError):
    """A call through the C ABI returned failure (message = sa_last_error())."""


class _Meta(C.Structure):  # struct sa_meta  <- reference src/bio/align.h:6-9
    _fields_ = [("off", C.c_int32), ("len", C.c_int32)]


class _Input(C.Structure):  # struct sa_input <- reference src/io/input.h:6-11
    _fields_ = [("seqs", C.c_void_p), ("meta", C.c_void_p), ("max", C.c_int32), ("num", C.c_int32)]


class _Output(C.Structure):  # struct sa_output <- reference src/io/output.h:10-15
    _fields_ = [("matrix", C.c_void_p), ("seqs", C.c_void_p), ("dim", C.c_size_t), ("triangular", C.c_bool)]


class _Scoring(C.Structure):  # struct sa_scoring
    _fields_ = [("method", C.c_int32), ("gap_pen", C.c_int32), ("gap_opn", C.c_int32), ("gap_ext", C.c_int32),
                ("lut", C.c_int32 * LUT_SIZE), ("sub", C.c_int32 * (SUB_DIM * SUB_DIM))]


#: every symbol include/seqalign_hip.h declares (tests check the .so exports exactly these)
ABI_SYMBOLS = (
    "sa_hip_memory", "sa_hip_align", "sa_hip_filter", "sa_ctx_create", "sa_ctx_destroy", "sa_ctx_pairs", "sa_pairs_cells",
    "sa_ctx_align_range", "sa_ctx_align_range16", "sa_ctx_token_tiles", "sa_ctx_scores_fit16", "sa_hip_widen16", "sa_ctx_expand_full", "sa_pairs_partition", "sa_ctx_timing", "sa_ctx_timing_read",
    "sa_matrix_load", "sa_matrix_count", "sa_matrix_name", "sa_matrix_is_nucleotide", "sa_method_parse",
    "sa_method_name", "sa_method_gap_kind", "sa_hip_device_count", "sa_hip_device_name", "sa_last_error",
    "sa_abi_version",
    "sa_hip_last_align_seconds", "sa_ctx_align_host", "sa_hip_host_register", "sa_hip_host_unregister",
    "sa_ctx_share_elems", "sa_ctx_align_share", "sa_ctx_place_shares", "sa_hip_last_align_breakdown", "sa_ctx_leave_room", "sa_hip_set_progress",
    "sa_hip_last_align_path",
    "sa_zjob_create", "sa_zjob_destroy", "sa_zjob_tiles_per_row", "sa_zjob_tile_row", "sa_zjob_stats", "sa_zjob_next", "sa_zjob_align_seconds", "sa_hip_tiles_begin",
    "sa_ctx_neighbors", "sa_hip_neighbors", "sa_zjob_neighbors", "sa_hip_last_neighbors_seconds",
    "sa_ctx_alignments", "sa_hip_alignments", "sa_alns_records", "sa_alns_cigar", "sa_alns_count", "sa_alns_destroy",
    "sa_hip_last_alignments_seconds", "sa_hip_last_alignments_breakdown",
    "sa_norm_value", "sa_ctx_denominators", "sa_ctx_normalize", "sa_zjob_normalize", "sa_hip_neighbors_norm", "sa_hip_edges_norm",
    "sa_hip_linkage_norm", "sa_hip_select_norm", "sa_hip_edges_at_rank_norm", "sa_hip_linkage_with_ranks_norm", "sa_hip_last_normalize_seconds",
    "sa_ctx_edge_offsets", "sa_ctx_edge_fill", "sa_hip_edges", "sa_zjob_edges", "sa_edges_offsets", "sa_edges_index", "sa_edges_score",
    "sa_edges_destroy", "sa_hip_last_edges_seconds",
    "sa_linkage_scratch_bytes", "sa_ctx_linkage", "sa_hip_linkage", "sa_zjob_linkage", "sa_linkage_pairs", "sa_linkage_score",
    "sa_linkage_destroy", "sa_hip_last_linkage_seconds", "sa_hip_last_linkage_rounds", "sa_linkage_labels", "sa_linkage_merges",
    "sa_select_scratch_bytes", "sa_score_rank", "sa_ctx_select", "sa_hip_select", "sa_zjob_select", "sa_hip_edges_at_rank",
    "sa_hip_linkage_with_ranks", "sa_hip_last_select_seconds",
    "sa_pid_value", "sa_ctx_identity_range", "sa_hip_identity", "sa_zjob_identity", "sa_hip_neighbors_pid", "sa_hip_edges_pid",
    "sa_hip_linkage_pid", "sa_hip_select_pid", "sa_hip_edges_at_rank_pid", "sa_hip_linkage_with_ranks_pid", "sa_hip_last_identity_seconds",
    "sa_agglo_scratch_bytes", "sa_ctx_agglomerate", "sa_hip_agglomerate", "sa_hip_agglomerate_with_ranks", "sa_zjob_agglomerate",
    "sa_agglo_labels", "sa_hip_last_agglomerate_seconds", "sa_hip_last_agglomerate_rescans",
    "sa_ctx_create_search", "sa_ctx_search_db", "sa_ctx_search_queries", "sa_search_scratch_bytes", "sa_ctx_search_range",
    "sa_hits_scratch_bytes", "sa_ctx_hits", "sa_hip_search", "sa_hip_last_search_seconds", "sa_hip_last_search_breakdown",
    "sa_ctx_normalize_rect", "sa_ctx_identity_rect", "sa_ctx_hits_take", "sa_hip_search_norm", "sa_hip_search_pid",
    "sa_hip_last_search_quantity_seconds",
    "sa_hits_above_scratch_bytes", "sa_ctx_hits_above_offsets", "sa_ctx_hits_above_fill", "sa_hip_search_above", "sa_hitlist_offsets",
    "sa_hitlist_index", "sa_hitlist_value", "sa_hitlist_score", "sa_hitlist_destroy", "sa_hip_last_search_above_seconds",
    "sa_dna_complement", "sa_reverse_complement", "sa_ctx_create_search_strands", "sa_ctx_search_strands", "sa_ctx_strand_fold",
    "sa_ctx_hits_strand", "sa_ctx_hits_above_strand", "sa_hip_search_strands", "sa_hip_search_above_strands", "sa_hitlist_strand",
    "sa_hip_last_search_strands_seconds",
    "sa_ctx_fit_rect", "sa_ctx_fit_pairs", "sa_ctx_fit_alignments", "sa_hip_search_fit", "sa_hip_last_search_fit_seconds",
)


class _Norm(C.Structure):  # struct sa_norm
    _fields_ = [("source", C.c_int32), ("rule", C.c_int32), ("denominators", C.c_void_p)]


class _IdentityOut(C.Structure):  # struct sa_identity_out
    _fields_ = [("score", C.c_void_p), ("identities", C.c_void_p), ("columns", C.c_void_p), ("pid", C.c_void_p), ("denom", C.c_int32)]


class _FitOut(C.Structure):  # struct sa_fit_out
    _fields_ = [("score", C.c_void_p), ("db_begin", C.c_void_p), ("db_end", C.c_void_p), ("identities", C.c_void_p), ("columns", C.c_void_p),
                ("pid", C.c_void_p), ("denom", C.c_int32)]


def library_path() -> pathlib.Path:
    return _LIB_PATH


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  The PyTorch-ROCm wheel ships a private libamdhip64.so that its
    libraries request by the un-versioned file name, so it does not unify with /opt/rocm's copy by
    soname; two runtimes in one process leave the second without devices.  When torch is installed
    but not imported yet, bring ITS runtime in first so that libseqalign_hip.so (NEEDED
    libamdhip64.so.7) and a later `import torch` resolve to the same object.  A plain C host links
    /opt/rocm's runtime and never sees this."""
    if "torch" in sys.modules or os.environ.get("SA_HIP_NO_TORCH_RUNTIME"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    cand = pathlib.Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if cand.exists():
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)


def load_library() -> C.CDLL:
    """Load libseqalign_hip.so (built in-tree by __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise AlignError(f"{_LIB_PATH} is missing: run `python __graft_entry__.py` (hipcc, gfx950) first; "
                         "there is no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(str(_LIB_PATH))
    lib.sa_hip_memory.argtypes = [C.c_size_t]
    lib.sa_hip_memory.restype = C.c_bool
    lib.sa_hip_align.argtypes = [_Input, _Output, C.POINTER(_Scoring)]
    lib.sa_hip_align.restype = C.c_bool
    lib.sa_hip_filter.argtypes = [_Input, C.c_float, C.c_void_p]
    lib.sa_hip_filter.restype = C.c_int32
    lib.sa_ctx_create.argtypes = [C.c_int, _Input, C.POINTER(_Scoring)]
    lib.sa_ctx_create.restype = C.c_void_p
    lib.sa_ctx_destroy.argtypes = [C.c_void_p]
    lib.sa_ctx_destroy.restype = None
    lib.sa_ctx_pairs.argtypes = [C.c_void_p]
    lib.sa_ctx_pairs.restype = C.c_int64
    lib.sa_pairs_cells.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
    lib.sa_pairs_cells.restype = C.c_int64
    lib.sa_ctx_align_range.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.sa_ctx_align_range.restype = C.c_int
    lib.sa_ctx_token_tiles.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.sa_ctx_token_tiles.restype = C.c_int
    lib.sa_ctx_align_range16.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.sa_ctx_align_range16.restype = C.c_int
    lib.sa_ctx_scores_fit16.argtypes = [C.c_void_p]
    lib.sa_ctx_scores_fit16.restype = C.c_int
    lib.sa_hip_widen16.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sa_hip_widen16.restype = C.c_int
    lib.sa_ctx_expand_full.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_expand_full.restype = C.c_int
    lib.sa_pairs_partition.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_int64)]
    lib.sa_pairs_partition.restype = C.c_int
    lib.sa_ctx_timing.argtypes = [C.c_void_p, C.c_int]
    lib.sa_ctx_timing.restype = None
    lib.sa_ctx_timing_read.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.sa_ctx_timing_read.restype = C.c_int
    lib.sa_matrix_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sa_matrix_load.restype = C.c_int
    lib.sa_matrix_count.restype = C.c_int
    lib.sa_matrix_name.argtypes = [C.c_int]
    lib.sa_matrix_name.restype = C.c_char_p
    lib.sa_matrix_is_nucleotide.argtypes = [C.c_int]
    lib.sa_matrix_is_nucleotide.restype = C.c_int
    lib.sa_method_parse.argtypes = [C.c_char_p]
    lib.sa_method_parse.restype = C.c_int
    lib.sa_method_name.argtypes = [C.c_int]
    lib.sa_method_name.restype = C.c_char_p
    lib.sa_method_gap_kind.argtypes = [C.c_int]
    lib.sa_method_gap_kind.restype = C.c_int
    lib.sa_hip_device_count.restype = C.c_int
    lib.sa_hip_device_name.argtypes = [C.c_int]
    lib.sa_hip_device_name.restype = C.c_char_p
    lib.sa_last_error.restype = C.c_char_p
    lib.sa_abi_version.restype = C.c_int
    lib.sa_hip_last_align_seconds.restype = C.c_double
    lib.sa_hip_last_align_path.restype = C.c_int
    lib.sa_ctx_align_host.argtypes = [C.c_void_p, C.c_int64, C.c_int64, _Output, C.POINTER(C.c_double)]
    lib.sa_ctx_align_host.restype = C.c_int
    lib.sa_hip_host_register.argtypes = [C.c_void_p, C.c_size_t]
    lib.sa_hip_host_register.restype = C.c_int
    lib.sa_hip_host_unregister.argtypes = [C.c_void_p]
    lib.sa_hip_host_unregister.restype = C.c_int
    lib.sa_hip_last_align_breakdown.argtypes = [C.POINTER(C.c_double), C.c_int]
    lib.sa_hip_last_align_breakdown.restype = C.c_int
    lib.sa_hip_set_progress.argtypes = [C.c_void_p, C.c_void_p]
    lib.sa_hip_set_progress.restype = None
    lib.sa_ctx_leave_room.argtypes = [C.c_void_p, C.c_int]
    lib.sa_ctx_leave_room.restype = None
    lib.sa_ctx_share_elems.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int]
    lib.sa_ctx_share_elems.restype = C.c_int64
    lib.sa_ctx_align_share.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sa_ctx_align_share.restype = C.c_int
    lib.sa_ctx_place_shares.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sa_ctx_place_shares.restype = C.c_int
    lib.sa_zjob_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_int]
    lib.sa_zjob_create.restype = C.c_void_p
    lib.sa_zjob_destroy.argtypes = [C.c_void_p]
    lib.sa_zjob_destroy.restype = None
    lib.sa_zjob_tiles_per_row.argtypes = [C.c_void_p]
    lib.sa_zjob_tiles_per_row.restype = C.c_size_t
    lib.sa_zjob_tile_row.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.sa_zjob_tile_row.restype = C.c_int
    lib.sa_zjob_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sa_zjob_stats.restype = None
    lib.sa_zjob_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.sa_zjob_next.restype = C.c_int
    lib.sa_zjob_align_seconds.argtypes = [C.c_void_p]
    lib.sa_zjob_align_seconds.restype = C.c_double
    lib.sa_hip_tiles_begin.argtypes = [_Input, C.POINTER(_Scoring), C.c_size_t, C.c_int]
    lib.sa_hip_tiles_begin.restype = C.c_void_p
    lib.sa_ctx_neighbors.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_neighbors.restype = C.c_int
    lib.sa_hip_neighbors.argtypes = [_Input, C.POINTER(_Scoring), C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_hip_neighbors.restype = C.c_bool
    lib.sa_zjob_neighbors.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_zjob_neighbors.restype = C.c_int
    lib.sa_hip_last_neighbors_seconds.restype = C.c_double
    lib.sa_ctx_alignments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sa_ctx_alignments.restype = C.c_void_p
    lib.sa_hip_alignments.argtypes = [_Input, C.POINTER(_Scoring), C.c_void_p, C.c_void_p, C.c_int64]
    lib.sa_hip_alignments.restype = C.c_void_p
    lib.sa_alns_records.argtypes = [C.c_void_p]
    lib.sa_alns_records.restype = C.c_void_p
    lib.sa_alns_cigar.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.sa_alns_cigar.restype = C.c_void_p
    lib.sa_alns_count.argtypes = [C.c_void_p]
    lib.sa_alns_count.restype = C.c_int64
    lib.sa_alns_destroy.argtypes = [C.c_void_p]
    lib.sa_alns_destroy.restype = None
    lib.sa_hip_last_alignments_seconds.restype = C.c_double
    lib.sa_hip_last_alignments_breakdown.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.sa_hip_last_alignments_breakdown.restype = None
    lib.sa_ctx_edge_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_ctx_edge_offsets.restype = C.c_int
    lib.sa_ctx_edge_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_edge_fill.restype = C.c_int
    lib.sa_hip_edges.argtypes = [_Input, C.POINTER(_Scoring), C.c_int32]
    lib.sa_hip_edges.restype = C.c_void_p
    lib.sa_zjob_edges.argtypes = [C.c_void_p, C.c_int32]
    lib.sa_zjob_edges.restype = C.c_void_p
    lib.sa_edges_offsets.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.sa_edges_offsets.restype = C.c_void_p
    lib.sa_edges_index.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.sa_edges_index.restype = C.c_void_p
    lib.sa_edges_score.argtypes = [C.c_void_p]
    lib.sa_edges_score.restype = C.c_void_p
    lib.sa_edges_destroy.argtypes = [C.c_void_p]
    lib.sa_edges_destroy.restype = None
    lib.sa_hip_last_edges_seconds.restype = C.c_double
    lib.sa_linkage_scratch_bytes.argtypes = [C.c_int32]
    lib.sa_linkage_scratch_bytes.restype = C.c_size_t
    lib.sa_ctx_linkage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_linkage.restype = C.c_int
    lib.sa_hip_linkage.argtypes = [_Input, C.POINTER(_Scoring)]
    lib.sa_hip_linkage.restype = C.c_void_p
    lib.sa_zjob_linkage.argtypes = [C.c_void_p]
    lib.sa_zjob_linkage.restype = C.c_void_p
    lib.sa_linkage_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.sa_linkage_pairs.restype = C.c_void_p
    lib.sa_linkage_score.argtypes = [C.c_void_p]
    lib.sa_linkage_score.restype = C.c_void_p
    lib.sa_linkage_destroy.argtypes = [C.c_void_p]
    lib.sa_linkage_destroy.restype = None
    lib.sa_hip_last_linkage_seconds.restype = C.c_double
    lib.sa_hip_last_linkage_rounds.restype = C.c_int
    lib.sa_linkage_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.sa_linkage_labels.restype = C.c_int32
    lib.sa_linkage_merges.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_linkage_merges.restype = C.c_int
    lib.sa_select_scratch_bytes.argtypes = [C.c_int32]
    lib.sa_select_scratch_bytes.restype = C.c_size_t
    lib.sa_score_rank.argtypes = [C.c_int64, C.c_double]
    lib.sa_score_rank.restype = C.c_int64
    lib.sa_ctx_select.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_select.restype = C.c_int
    lib.sa_hip_select.argtypes = [_Input, C.POINTER(_Scoring), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_hip_select.restype = C.c_bool
    lib.sa_zjob_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_zjob_select.restype = C.c_int
    lib.sa_hip_edges_at_rank.argtypes = [_Input, C.POINTER(_Scoring), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.sa_hip_edges_at_rank.restype = C.c_void_p
    lib.sa_hip_linkage_with_ranks.argtypes = [_Input, C.POINTER(_Scoring), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_hip_linkage_with_ranks.restype = C.c_void_p
    lib.sa_hip_last_select_seconds.restype = C.c_double
    lib.sa_norm_value.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.sa_norm_value.restype = C.c_int32
    lib.sa_ctx_denominators.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_ctx_denominators.restype = C.c_int
    lib.sa_ctx_normalize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_ctx_normalize.restype = C.c_int
    lib.sa_zjob_normalize.argtypes = [C.c_void_p, C.POINTER(_Norm)]
    lib.sa_zjob_normalize.restype = C.c_int
    lib.sa_hip_neighbors_norm.argtypes = lib.sa_hip_neighbors.argtypes + [C.POINTER(_Norm)]
    lib.sa_hip_neighbors_norm.restype = C.c_bool
    lib.sa_hip_edges_norm.argtypes = lib.sa_hip_edges.argtypes + [C.POINTER(_Norm)]
    lib.sa_hip_edges_norm.restype = C.c_void_p
    lib.sa_hip_linkage_norm.argtypes = lib.sa_hip_linkage.argtypes + [C.POINTER(_Norm)]
    lib.sa_hip_linkage_norm.restype = C.c_void_p
    lib.sa_hip_select_norm.argtypes = lib.sa_hip_select.argtypes + [C.POINTER(_Norm)]
    lib.sa_hip_select_norm.restype = C.c_bool
    lib.sa_hip_edges_at_rank_norm.argtypes = lib.sa_hip_edges_at_rank.argtypes + [C.POINTER(_Norm)]
    lib.sa_hip_edges_at_rank_norm.restype = C.c_void_p
    lib.sa_hip_linkage_with_ranks_norm.argtypes = lib.sa_hip_linkage_with_ranks.argtypes + [C.POINTER(_Norm)]
    lib.sa_hip_linkage_with_ranks_norm.restype = C.c_void_p
    lib.sa_hip_last_normalize_seconds.restype = C.c_double
    lib.sa_pid_value.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.sa_pid_value.restype = C.c_int32
    lib.sa_ctx_identity_range.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(_IdentityOut), C.c_void_p]
    lib.sa_ctx_identity_range.restype = C.c_int
    lib.sa_hip_identity.argtypes = [_Input, C.POINTER(_Scoring), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_hip_identity.restype = C.c_bool
    lib.sa_zjob_identity.argtypes = [C.c_void_p, C.c_int32]
    lib.sa_zjob_identity.restype = C.c_int
    lib.sa_hip_neighbors_pid.argtypes = lib.sa_hip_neighbors.argtypes + [C.c_int32]
    lib.sa_hip_neighbors_pid.restype = C.c_bool
    lib.sa_hip_edges_pid.argtypes = lib.sa_hip_edges.argtypes + [C.c_int32]
    lib.sa_hip_edges_pid.restype = C.c_void_p
    lib.sa_hip_linkage_pid.argtypes = lib.sa_hip_linkage.argtypes + [C.c_int32]
    lib.sa_hip_linkage_pid.restype = C.c_void_p
    lib.sa_hip_select_pid.argtypes = lib.sa_hip_select.argtypes + [C.c_int32]
    lib.sa_hip_select_pid.restype = C.c_bool
    lib.sa_hip_edges_at_rank_pid.argtypes = lib.sa_hip_edges_at_rank.argtypes + [C.c_int32]
    lib.sa_hip_edges_at_rank_pid.restype = C.c_void_p
    lib.sa_hip_linkage_with_ranks_pid.argtypes = lib.sa_hip_linkage_with_ranks.argtypes + [C.c_int32]
    lib.sa_hip_linkage_with_ranks_pid.restype = C.c_void_p
    lib.sa_hip_last_identity_seconds.restype = C.c_double
    lib.sa_agglo_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.sa_agglo_scratch_bytes.restype = C.c_size_t
    lib.sa_ctx_agglomerate.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_agglomerate.restype = C.c_int
    lib.sa_hip_agglomerate.argtypes = [_Input, C.POINTER(_Scoring), C.c_int32, C.POINTER(_Norm), C.POINTER(C.c_int32)]
    lib.sa_hip_agglomerate.restype = C.c_void_p
    lib.sa_hip_agglomerate_with_ranks.argtypes = lib.sa_hip_agglomerate.argtypes + [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_hip_agglomerate_with_ranks.restype = C.c_void_p
    lib.sa_zjob_agglomerate.argtypes = [C.c_void_p, C.c_int32]
    lib.sa_zjob_agglomerate.restype = C.c_void_p
    lib.sa_agglo_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.sa_agglo_labels.restype = C.c_int32
    lib.sa_hip_last_agglomerate_seconds.restype = C.c_double
    lib.sa_hip_last_agglomerate_rescans.restype = C.c_int64
    lib.sa_ctx_create_search.argtypes = [C.c_int, _Input, _Input, C.POINTER(_Scoring)]
    lib.sa_ctx_create_search.restype = C.c_void_p
    lib.sa_ctx_search_db.argtypes = [C.c_void_p]
    lib.sa_ctx_search_db.restype = C.c_int32
    lib.sa_ctx_search_queries.argtypes = [C.c_void_p]
    lib.sa_ctx_search_queries.restype = C.c_int32
    lib.sa_search_scratch_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.sa_search_scratch_bytes.restype = C.c_size_t
    lib.sa_ctx_search_range.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_search_range.restype = C.c_int
    lib.sa_hits_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.sa_hits_scratch_bytes.restype = C.c_size_t
    lib.sa_ctx_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_hits.restype = C.c_int
    lib.sa_hip_search.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_hip_search.restype = C.c_bool
    lib.sa_hip_last_search_seconds.restype = C.c_double
    lib.sa_hip_last_search_breakdown.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.sa_hip_last_search_breakdown.restype = None
    lib.sa_ctx_normalize_rect.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sa_ctx_normalize_rect.restype = C.c_int
    lib.sa_ctx_identity_rect.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_IdentityOut), C.c_void_p]
    lib.sa_ctx_identity_rect.restype = C.c_int
    lib.sa_ctx_hits_take.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_hits_take.restype = C.c_int
    lib.sa_hip_search_norm.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_int32] + [C.c_void_p] * 5 + [C.POINTER(_Norm)]
    lib.sa_hip_search_norm.restype = C.c_bool
    lib.sa_hip_search_pid.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
    lib.sa_hip_search_pid.restype = C.c_bool
    lib.sa_hip_last_search_quantity_seconds.restype = C.c_double
    lib.sa_ctx_fit_rect.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_FitOut), C.c_void_p]
    lib.sa_ctx_fit_rect.restype = C.c_int
    lib.sa_ctx_fit_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_FitOut), C.c_void_p]
    lib.sa_ctx_fit_pairs.restype = C.c_int
    lib.sa_ctx_fit_alignments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sa_ctx_fit_alignments.restype = C.c_void_p
    lib.sa_hip_search_fit.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_int32, C.c_int32] + [C.c_void_p] * 7
    lib.sa_hip_search_fit.restype = C.c_bool
    lib.sa_hip_last_search_fit_seconds.restype = C.c_double
    lib.sa_hits_above_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.sa_hits_above_scratch_bytes.restype = C.c_size_t
    lib.sa_ctx_hits_above_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_hits_above_offsets.restype = C.c_int
    lib.sa_ctx_hits_above_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    lib.sa_ctx_hits_above_fill.restype = C.c_int
    lib.sa_hip_search_above.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_int32, C.POINTER(_Norm), C.POINTER(C.c_int32)]
    lib.sa_hip_search_above.restype = C.c_void_p
    lib.sa_hitlist_offsets.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.sa_hitlist_offsets.restype = C.c_void_p
    lib.sa_hitlist_index.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.sa_hitlist_index.restype = C.c_void_p
    lib.sa_hitlist_value.argtypes = [C.c_void_p]
    lib.sa_hitlist_value.restype = C.c_void_p
    lib.sa_hitlist_score.argtypes = [C.c_void_p]
    lib.sa_hitlist_score.restype = C.c_void_p
    lib.sa_hitlist_destroy.argtypes = [C.c_void_p]
    lib.sa_hitlist_destroy.restype = None
    lib.sa_hip_last_search_above_seconds.restype = C.c_double
    lib.sa_dna_complement.argtypes = [C.c_void_p]
    lib.sa_dna_complement.restype = None
    lib.sa_reverse_complement.argtypes = [_Input, C.c_void_p, C.POINTER(_Scoring), C.c_void_p]
    lib.sa_reverse_complement.restype = C.c_bool
    lib.sa_ctx_create_search_strands.argtypes = [C.c_int, _Input, _Input, C.POINTER(_Scoring), C.c_void_p]
    lib.sa_ctx_create_search_strands.restype = C.c_void_p
    lib.sa_ctx_search_strands.argtypes = [C.c_void_p]
    lib.sa_ctx_search_strands.restype = C.c_int32
    lib.sa_ctx_strand_fold.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4
    lib.sa_ctx_strand_fold.restype = C.c_int
    lib.sa_ctx_hits_strand.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_hits_strand.restype = C.c_int
    lib.sa_ctx_hits_above_strand.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sa_ctx_hits_above_strand.restype = C.c_int
    lib.sa_hip_search_strands.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.POINTER(_Norm),
                                                                                                                 C.POINTER(C.c_int32)]
    lib.sa_hip_search_strands.restype = C.c_bool
    lib.sa_hip_last_search_strands_seconds.restype = C.c_double
    lib.sa_hip_search_above_strands.argtypes = [_Input, _Input, C.POINTER(_Scoring), C.c_void_p, C.c_int32, C.POINTER(_Norm), C.POINTER(C.c_int32)]
    lib.sa_hip_search_above_strands.restype = C.c_void_p
    lib.sa_hitlist_strand.argtypes = [C.c_void_p]
    lib.sa_hitlist_strand.restype = C.c_void_p
    _lib = lib
    return lib


def _err() -> str:
    return (load_library().sa_last_error() or b"").decode(errors="replace")


def device_count() -> int:
    return int(load_library().sa_hip_device_count())


def last_align_seconds() -> float:
    """launch/copy phase of the last hip_align call (the reference's bench_align bracket, seqalign_cuda.c:182,292)"""
    return float(load_library().sa_hip_last_align_seconds())


def last_align_path() -> str:
    """schedule of the last hip_align call: "slices" (every device delivers a contiguous slice; one device: the whole
    range) or "gather" (dense shares + RCCL all-gather + placement on every device)"""
    return {0: "none", 1: "slices", 2: "gather"}[int(load_library().sa_hip_last_align_path())]


def last_align_breakdown() -> dict:
    """milliseconds of the last hip_align call by stage (enum sa_breakdown): set-up itemised, then the phase"""
    names = ("encode_ms", "device_ms", "upload_ms", "code_objects_ms", "pin_ms", "plan_ms", "arrange_ms", "phase_ms", "total_ms")
    buf = (C.c_double * len(names))()
    n = load_library().sa_hip_last_align_breakdown(buf, len(names))
    return {names[k]: float(buf[k]) for k in range(n)}


PROGRESS_FN = C.CFUNCTYPE(None, C.c_double, C.c_void_p)
_progress_keepalive = None


def set_progress(fn) -> None:
    """fn(fraction) while hip_align / Context.align_host waits for the device (the reference's progress side channel,
    seqalign_cuda.c:286-289); None switches it off"""
    global _progress_keepalive
    lib = load_library()
    if fn is None:
        lib.sa_hip_set_progress(None, None)
        _progress_keepalive = None
        return
    _progress_keepalive = PROGRESS_FN(lambda fraction, _user: fn(float(fraction)))
    lib.sa_hip_set_progress(C.cast(_progress_keepalive, C.c_void_p), None)


def device_name(device: int = 0) -> str:
    name = load_library().sa_hip_device_name(device)
    if not name:
        raise AlignError(f"no HIP device {device}")
    return name.decode()


def matrix_names() -> list[str]:
    lib = load_library()
    return [lib.sa_matrix_name(k).decode() for k in range(lib.sa_matrix_count())]


def method_names() -> list[str]:
    lib = load_library()
    return [lib.sa_method_name(k).decode() for k in range(3)]


def pair_count(n: int) -> int:
    """reference src/util/macros.h:13 `alignments(n)`"""
    return n * (n - 1) // 2


# --------------------------------------------------------------------------------------------
@dataclass
class SequenceStore:
    """The reference's `struct input` (src/io/input.h:6-11): one NUL-separated uppercase blob + meta[]."""
    blob: np.ndarray            # uint8, sum(len+1) bytes
    meta: np.ndarray            # int32 [num, 2] = (off, len)
    num: int
    max: int

    @classmethod
    def from_sequences(cls, seqs: Iterable[bytes | str]) -> "SequenceStore":
        # what input_load builds after a parser ran (src/io/input.c:68-81): sequences back to back,
        # each NUL-terminated; parsers upper-case residues (src/io/source/fasta.c:51)
        items = [(s.encode() if isinstance(s, str) else bytes(s)).upper() for s in seqs]
        lens = np.fromiter((len(s) for s in items), dtype=np.int64, count=len(items))
        total = int(lens.sum()) + len(items)
        if total > np.iinfo(np.int32).max:
            raise AlignError("sequence store exceeds 2 GiB")
        blob = np.frombuffer(b"\0".join(items) + b"\0", dtype=np.uint8).copy()
        offs = np.zeros(len(items), dtype=np.int64)
        if len(items):
            offs[1:] = np.cumsum(lens[:-1] + 1)
        meta = np.stack([offs, lens], axis=1).astype(np.int32)
        return cls(blob=blob, meta=np.ascontiguousarray(meta), num=len(items), max=int(lens.max()) if len(items) else 0)

    def sequence(self, k: int) -> bytes:
        off, ln = self.meta[k]
        return self.blob[off:off + ln].tobytes()

    def select(self, keep: Sequence[int]) -> "SequenceStore":
        return SequenceStore.from_sequences(self.sequence(int(k)) for k in keep)

    def prefix(self, n: int) -> "SequenceStore":
        return self.select(range(n))

    def _as_c(self) -> _Input:
        return _Input(self.blob.ctypes.data, self.meta.ctypes.data, self.max, self.num)

    @property
    def pairs(self) -> int:
        return pair_count(self.num)

    def cells(self, start: int = 0, count: Optional[int] = None) -> int:
        """DP cells (sum len_i*len_j) of packed pair range [start, start+count) -- GCUPS numerator."""
        count = self.pairs - start if count is None else count
        v = int(load_library().sa_pairs_cells(self.meta.ctypes.data, self.num, start, count))
        if v < 0:
            raise AlignError("bad pair range")
        return v

    def partition(self, parts: int) -> list[int]:
        """Cut points of `parts` contiguous packed-index ranges of near-equal DP work (multi-GPU sharding)."""
        b = (C.c_int64 * (parts + 1))()
        if load_library().sa_pairs_partition(self.meta.ctypes.data, self.num, parts, b):
            raise AlignError(_err())
        return list(b)


@dataclass
class Scoring:
    """The reference's scoring globals (src/bio/align.h:11-19); gaps in STORED (negated) form."""
    method: int
    gap_pen: int = 0
    gap_opn: int = 0
    gap_ext: int = 0
    lut: np.ndarray = field(default_factory=lambda: np.full(LUT_SIZE, -1, np.int32))
    sub: np.ndarray = field(default_factory=lambda: np.zeros(SUB_DIM * SUB_DIM, np.int32))
    matrix_name: str = ""

    @classmethod
    def from_names(cls, method: str, matrix: str, gap_pen: Optional[int] = None, gap_open: Optional[int] = None,
                   gap_extend: Optional[int] = None, equal_affine_to_nw: bool = True) -> "Scoring":
        """`-a METHOD -m MATRIX (-p N | -s N -e N)` with the reference's validation rules.

        parse_align src/bio/align.c:87-96; parse_matrix src/bio/matrices.c:44-58; gap values are given
        positive and stored negated (src/bio/align.c:127-128); -p only with a linear method, -s/-e only with
        an affine one and both required (src/bio/align.c:130-142,170-201); Gotoh with open == extend becomes
        NW with that penalty (validate_ga, src/bio/method/ga.c:70-88, the -F answer)."""
        lib = load_library()
        m = lib.sa_method_parse(method.encode())
        if m < 0:
            raise AlignError("Invalid alignment method")
        lut = np.empty(LUT_SIZE, np.int32)
        sub = np.empty(SUB_DIM * SUB_DIM, np.int32)
        if lib.sa_matrix_load(matrix.encode(), lut.ctypes.data_as(C.POINTER(C.c_int32)),
                              sub.ctypes.data_as(C.POINTER(C.c_int32))):
            raise AlignError("Invalid substitution matrix name")
        for name, v in (("gap_pen", gap_pen), ("gap_open", gap_open), ("gap_extend", gap_extend)):
            if v is not None and not (0 <= int(v) <= 2**31 - 1):
                raise AlignError("Gap values must be positive integers")
        kind = lib.sa_method_gap_kind(m)
        if kind == GAP_LINEAR:
            if gap_open is not None or gap_extend is not None:
                raise AlignError("Affine gaps cannot be set for non-affine methods")
            if gap_pen is None:
                raise AlignError("Linear gap penalty (-p) is required")
            return cls(m, gap_pen=-int(gap_pen), lut=lut, sub=sub, matrix_name=matrix.lower())
        if gap_pen is not None:
            raise AlignError("Gap penalty cannot be set for non-linear methods")
        if gap_open is None or gap_extend is None:
            raise AlignError("Affine gap open (-s) and extend (-e) are required")
        if m == METHOD_GA and gap_open == gap_extend and equal_affine_to_nw:
            return cls(METHOD_NW, gap_pen=-int(gap_open), gap_opn=SCORE_MIN, gap_ext=SCORE_MIN, lut=lut, sub=sub,
                       matrix_name=matrix.lower())
        return cls(m, gap_opn=-int(gap_open), gap_ext=-int(gap_extend), lut=lut, sub=sub, matrix_name=matrix.lower())

    @property
    def method_name(self) -> str:
        return ("nw", "ga", "sw")[self.method]

    def _as_c(self) -> _Scoring:
        s = _Scoring(self.method, self.gap_pen, self.gap_opn, self.gap_ext)
        C.memmove(s.lut, np.ascontiguousarray(self.lut, np.int32).ctypes.data, 4 * LUT_SIZE)
        C.memmove(s.sub, np.ascontiguousarray(self.sub, np.int32).ctypes.data, 4 * SUB_DIM * SUB_DIM)
        return s


# --------------------------------------------------------------------------------------------
def hip_memory(nbytes: int) -> bool:
    """`cuda_memory` replacement (reference src/interface/seqalign_cuda.c:71-93)."""
    return bool(load_library().sa_hip_memory(int(nbytes)))


def hip_align(store: SequenceStore, scoring: Scoring, triangular: bool = False, write: bool = True) -> Optional[np.ndarray]:
    """`cuda_align` replacement (reference src/interface/seqalign_cuda.c:95-296).

    Returns the host matrix the reference would hand to its writer: packed triangular
    (pair i<j at j(j-1)/2+i) or full N x N symmetric with zero diagonal; None when write=False
    (the reference's -W: compute, copy nothing)."""
    lib = load_library()
    n = store.num
    matrix = None
    if write:
        # an anonymous zero-filled mapping like output_load's (output.c:55) -- page-aligned and not malloc's, so the library may
        # page-lock it for the call (it never locks memory malloc manages: DESIGN.md 9)
        import mmap
        elements = pair_count(n) if triangular else n * n
        matrix = np.frombuffer(mmap.mmap(-1, 4 * max(elements, 1)), dtype=np.int32)[:elements]
    out = _Output(matrix.ctypes.data if matrix is not None else None, None, n, bool(triangular))
    sc = scoring._as_c()
    if not lib.sa_hip_align(store._as_c(), out, C.byref(sc)):
        raise AlignError(_err())
    if matrix is None:
        return None
    return matrix if triangular else matrix.reshape(n, n)


NORM_SELF, NORM_LENGTH = 0, 1        # SA_NORM_SELF, SA_NORM_LENGTH: where the per-sequence denominator comes from
NORM_MIN, NORM_MAX, NORM_MEAN = 0, 1, 2  # SA_NORM_MIN, SA_NORM_MAX, SA_NORM_MEAN: how d[i] and d[j] combine
NORM_SCALE = 1000000                 # SA_NORM_SCALE: a normalised score is in parts per million


class Norm:
    """struct sa_norm: normalised scores for the selections -- source NORM_SELF (self-scores) or NORM_LENGTH (lengths), rule
    NORM_MIN / NORM_MAX / NORM_MEAN.  Which values are valid is the library's to say."""

    def __init__(self, source: int = NORM_SELF, rule: int = NORM_MIN):
        self.source, self.rule = int(source), int(rule)
        for v in (self.source, self.rule):
            if not -2**31 <= v < 2**31:
                raise AlignError(f"{v} is not an int32")

    def _as_c(self, n: int) -> tuple["_Norm", np.ndarray]:
        """the C struct and the host array that receives the denominators"""
        den = np.zeros(max(int(n), 1), np.int32)
        return _Norm(self.source, self.rule, den.ctypes.data), den

    def __repr__(self) -> str:
        return f"Norm(source={self.source}, rule={self.rule})"


def norm_value(s: int, di: int, dj: int, rule: int) -> int:
    """sa_norm_value (host only): the normalised value of score s under denominators di, dj -- floor division towards minus
    infinity in parts per million, saturated to int32; INT32_MIN for a denominator <= 0"""
    args = [int(s), int(di), int(dj), int(rule)]
    for v in args:
        if not -2**31 <= v < 2**31:
            raise AlignError(f"{v} is not an int32")
    got = int(load_library().sa_norm_value(*args))
    if args[3] not in (NORM_MIN, NORM_MAX, NORM_MEAN):  # (refused by the library: the message is its own)
        raise AlignError(_err())
    return got


def last_normalize_seconds() -> float:
    """device time of denominators + sweep in the last call with a norm / DeflateJob.normalize call"""
    return float(load_library().sa_hip_last_normalize_seconds())


PID_COLUMNS, PID_SHORTER, PID_LONGER, PID_MEAN = 0, 1, 2, 3  # SA_PID_*: what the identities are divided by


def _denom(denom) -> int:
    d = int(denom)
    if not -2**31 <= d < 2**31:
        raise AlignError(f"denom = {d} is not an int32")
    return d


def pid_value(identities: int, columns: int, len_i: int, len_j: int, denom: int) -> int:
    """sa_pid_value (host only): percent identity in parts per million -- floor(num / D) under `denom` (PID_COLUMNS, PID_SHORTER,
    PID_LONGER, PID_MEAN); INT32_MIN for D <= 0"""
    args = [int(identities), int(columns), int(len_i), int(len_j), int(denom)]
    for v in args:
        if not -2**31 <= v < 2**31:
            raise AlignError(f"{v} is not an int32")
    got = int(load_library().sa_pid_value(*args))
    if args[4] not in (PID_COLUMNS, PID_SHORTER, PID_LONGER, PID_MEAN):  # (refused by the library: the message is its own)
        raise AlignError(_err())
    return got


def hip_identity(store: SequenceStore, scoring: Scoring, denom: Optional[int] = None, identities: bool = True, columns: bool = True):
    """sa_hip_identity: identities and columns of the canonical alignment of every pair, and with a `denom` their percent identity
    in parts per million, as packed triangles (N (N - 1) / 2 int32) -- (identities, columns, pid), None for what was not asked
    for.  One forward sweep on the device, no traceback."""
    pairs = pair_count(store.num)
    ident = np.empty(max(pairs, 1), np.int32) if identities else None
    cols = np.empty(max(pairs, 1), np.int32) if columns else None
    pid = np.empty(max(pairs, 1), np.int32) if denom is not None else None
    sc = scoring._as_c()
    ptr = [None if a is None else a.ctypes.data for a in (ident, cols, pid)]
    if not load_library().sa_hip_identity(store._as_c(), C.byref(sc), _denom(0 if denom is None else denom), *ptr):
        raise AlignError(_err())
    return tuple(None if a is None else a[:pairs] for a in (ident, cols, pid))


def last_identity_seconds() -> float:
    """device time of the identity sweep in the last hip_identity / pid= selection / DeflateJob.identity call"""
    return float(load_library().sa_hip_last_identity_seconds())


def _quantity(base: str, norm: Optional[Norm], pid: Optional[int], n: int):
    """What a selection reads -- the scores (`base`), the scores normalised under `norm` (`base`_norm) or percent identity in
    parts per million under the denominator `pid` (`base`_pid): the library function, its trailing arguments, and what the
    result gains behind the plain tuple: the n denominators for a norm, nothing otherwise"""
    lib = load_library()
    if pid is not None:
        if norm is not None:
            raise AlignError("norm and pid exclude each other")
        return getattr(lib, base + "_pid"), (_denom(pid),), ()
    if norm is not None:
        cn, den = norm._as_c(n)
        return getattr(lib, base + "_norm"), (C.byref(cn),), (den[:n],)
    return getattr(lib, base), (), ()


def hip_neighbors(store: SequenceStore, scoring: Scoring, k: int, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_neighbors: the k best partners of every sequence, selected on the device -- (index, score), two (N, k) int32
    arrays; row r lists the c != r by score descending, then index ascending.  The matrix never leaves the device.
    1 <= k <= min(N - 1, NEIGHBORS_MAX).  With a norm: (index, score, denominators)."""
    n, k = store.num, int(k)
    if not -2**31 <= k < 2**31:
        raise AlignError(f"k = {k} is not an int32")
    rows = max(n, 1) * max(min(k, NEIGHBORS_MAX), 1)
    index, score = np.empty(rows, np.int32), np.empty(rows, np.int32)
    sc = scoring._as_c()
    fn, tail, den = _quantity("sa_hip_neighbors", norm, pid, n)
    if not fn(store._as_c(), C.byref(sc), k, index.ctypes.data, score.ctypes.data, *tail):
        raise AlignError(_err())
    return (index[:n * k].reshape(n, k), score[:n * k].reshape(n, k)) + den


def last_neighbors_seconds() -> float:
    """device time of the selection kernel in the last hip_neighbors / DeflateJob.neighbors call"""
    return float(load_library().sa_hip_last_neighbors_seconds())


def _min_score(min_score) -> int:
    t = int(min_score)
    if not -2**31 <= t < 2**31:
        raise AlignError(f"min_score = {t} is not an int32")
    return t


def _take_edges(lib, handle) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """copies of the three arrays a sa_edges handle owns; the handle is destroyed"""
    if not handle:
        raise AlignError(_err())
    try:
        num, count = C.c_int32(0), C.c_int64(0)
        off = lib.sa_edges_offsets(handle, C.byref(num))
        idx = lib.sa_edges_index(handle, C.byref(count))
        sco = lib.sa_edges_score(handle)
        e = count.value
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_int64)), (num.value + 1,)).copy()
        index = np.ctypeslib.as_array(C.cast(idx, C.POINTER(C.c_int32)), (e,)).copy() if e else np.zeros(0, np.int32)
        score = np.ctypeslib.as_array(C.cast(sco, C.POINTER(C.c_int32)), (e,)).copy() if e else np.zeros(0, np.int32)
    finally:
        lib.sa_edges_destroy(handle)
    return offsets, index, score


def hip_edges(store: SequenceStore, scoring: Scoring, min_score: int, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_edges: every pair that scores at least min_score, as the symmetric adjacency in CSR form, built on the device --
    (offsets int64[N + 1], index int32[E], score int32[E]); row r's columns are index[offsets[r]:offsets[r + 1]], ascending.
    The matrix never leaves the device.  Any int32 threshold is valid; with a norm or a pid it is in parts per million, and
    with a norm the result is (offsets, index, score, denominators)."""
    sc, t = scoring._as_c(), _min_score(min_score)
    fn, tail, den = _quantity("sa_hip_edges", norm, pid, store.num)
    return _take_edges(load_library(), fn(store._as_c(), C.byref(sc), t, *tail)) + den


def last_edges_seconds() -> float:
    """device time of count + scan + fill in the last hip_edges / DeflateJob.edges call"""
    return float(load_library().sa_hip_last_edges_seconds())


def _take_linkage(lib, handle) -> tuple[np.ndarray, np.ndarray]:
    """copies of the two arrays a sa_linkage handle owns; the handle is destroyed"""
    if not handle:
        raise AlignError(_err())
    try:
        merges = C.c_int32(0)
        prs = lib.sa_linkage_pairs(handle, C.byref(merges))
        sco = lib.sa_linkage_score(handle)
        m = merges.value
        pairs = np.ctypeslib.as_array(C.cast(prs, C.POINTER(C.c_int32)), (2 * m,)).copy() if m else np.zeros(0, np.int32)
        score = np.ctypeslib.as_array(C.cast(sco, C.POINTER(C.c_int32)), (m,)).copy() if m else np.zeros(0, np.int32)
    finally:
        lib.sa_linkage_destroy(handle)
    return pairs.reshape(m, 2), score


def hip_linkage(store: SequenceStore, scoring: Scoring, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_linkage: the single-linkage tree (the maximum spanning tree of the score matrix), built on the device --
    (pairs int32 (N - 1, 2) with lo < hi, score int32 (N - 1,)), sorted by score descending, then packed index ascending: the
    order in which single linkage joins clusters.  The matrix never leaves the device.  With a norm: (pairs, score, denominators)."""
    sc = scoring._as_c()
    fn, tail, den = _quantity("sa_hip_linkage", norm, pid, store.num)
    return _take_linkage(load_library(), fn(store._as_c(), C.byref(sc), *tail)) + den


def linkage_scratch_bytes(n: int) -> int:
    """sa_linkage_scratch_bytes: the device scratch memory Context.linkage needs for n sequences"""
    return int(load_library().sa_linkage_scratch_bytes(int(n)))


def last_linkage_seconds() -> float:
    """device time of rounds + sort in the last hip_linkage / DeflateJob.linkage call"""
    return float(load_library().sa_hip_last_linkage_seconds())


def last_linkage_rounds() -> int:
    """rounds of the last hip_linkage / DeflateJob.linkage call that found more than one component"""
    return int(load_library().sa_hip_last_linkage_rounds())


def _tree_arrays(pairs, score, n: int):
    n = int(n)
    if not 1 <= n < 2**31:
        raise AlignError(f"n = {n} is not a number of sequences")
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1)
    if pairs.size != 2 * (n - 1):
        raise AlignError(f"pairs holds {pairs.size} elements, a tree of {n} sequences has {2 * (n - 1)}")
    if score is not None:
        score = np.ascontiguousarray(score, np.int32).reshape(-1)
        if score.size != n - 1:
            raise AlignError(f"score holds {score.size} elements, a tree of {n} sequences has {n - 1}")
    return n, pairs, score


SELECT_MAX = 16  # SA_HIP_SELECT_MAX


def _ranks(ranks) -> np.ndarray:
    """the ranks of a select call as a contiguous int64 array; how many and which are valid is the library's to say"""
    try:
        return np.ascontiguousarray(np.asarray(ranks).reshape(-1), dtype=np.int64)
    except (OverflowError, TypeError, ValueError) as e:
        raise AlignError(f"ranks are not int64: {e}") from None


def _select_room(m: int) -> tuple[np.ndarray, np.ndarray]:
    """host arrays for value / below: room for a full call, so that a refused m never meets a short array"""
    room = max(m, SELECT_MAX)
    return np.zeros(room, np.int32), np.zeros(room, np.int64)


def score_rank(pairs: int, q: float) -> int:
    """sa_score_rank (host only): min(pairs - 1, int(q * pairs)) for 0 <= q <= 1; -1 for a NaN, a q outside [0, 1], pairs < 1"""
    return int(load_library().sa_score_rank(int(pairs), float(q)))


def select_scratch_bytes(m: int) -> int:
    """sa_select_scratch_bytes: the device scratch memory Context.select needs for m ranks (0 for an m outside 1 .. 16)"""
    return int(load_library().sa_select_scratch_bytes(int(m)))


def hip_select(store: SequenceStore, scoring: Scoring, ranks, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_select: for each rank k (up to 16, any order, duplicates allowed) into the ascending order of the N (N - 1) / 2
    pair scores, (values int32 (m,), below int64 (m,)): the k-th smallest score and the number of pairs strictly below it,
    selected on the device.  The matrix never leaves the device.  With a norm: (values, below, denominators)."""
    sc = scoring._as_c()
    r = _ranks(ranks)
    value, below = _select_room(len(r))
    fn, tail, den = _quantity("sa_hip_select", norm, pid, store.num)
    if not fn(store._as_c(), C.byref(sc), r.ctypes.data, len(r), value.ctypes.data, below.ctypes.data, *tail):
        raise AlignError(_err())
    return (value[:len(r)].copy(), below[:len(r)].copy()) + den


def hip_edges_at_rank(store: SequenceStore, scoring: Scoring, rank: int, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_edges_at_rank: one alignment, the score T at `rank` and the score graph at T from the same device matrix --
    (offsets, index, score) as hip_edges returns them, then min_score = T and below = the pairs under T; E = 2 (P - below).
    With a norm the denominators follow."""
    sc = scoring._as_c()
    cut, below = C.c_int32(0), C.c_int64(0)
    (rank,) = _ranks([rank])
    fn, tail, den = _quantity("sa_hip_edges_at_rank", norm, pid, store.num)
    edges = _take_edges(load_library(), fn(store._as_c(), C.byref(sc), int(rank), C.byref(cut), C.byref(below), *tail))
    return edges + (int(cut.value), int(below.value)) + den


def hip_linkage_with_ranks(store: SequenceStore, scoring: Scoring, ranks, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_linkage_with_ranks: one alignment, then hip_select's (values, below) for `ranks` and hip_linkage's (pairs, score)
    from the same device matrix -- (pairs, score, values, below); with a norm the denominators follow"""
    sc = scoring._as_c()
    r = _ranks(ranks)
    value, below = _select_room(len(r))
    fn, tail, den = _quantity("sa_hip_linkage_with_ranks", norm, pid, store.num)
    tree = _take_linkage(load_library(), fn(store._as_c(), C.byref(sc), r.ctypes.data, len(r), value.ctypes.data, below.ctypes.data, *tail))
    return tree + (value[:len(r)].copy(), below[:len(r)].copy()) + den


def last_select_seconds() -> float:
    """device time of the rounds in the last hip_select / DeflateJob.select / *_at_rank / *_with_ranks call"""
    return float(load_library().sa_hip_last_select_seconds())


def linkage_labels(pairs, score, n: int, min_score: int) -> tuple[np.ndarray, int]:
    """sa_linkage_labels (host only): (labels int32 (N,), clusters) -- labels[r] is the smallest index in r's connected
    component of the graph score >= min_score, from the tree alone.  Any int32 threshold is valid."""
    n, pairs, score = _tree_arrays(pairs, score, n)
    labels = np.empty(n, np.int32)
    clusters = load_library().sa_linkage_labels(pairs.ctypes.data, score.ctypes.data, n, _min_score(min_score), labels.ctypes.data)
    if clusters < 0:
        raise AlignError(_err())
    return labels, int(clusters)


AGGLO_COMPLETE, AGGLO_AVERAGE = 1, 2  # SA_AGGLO_COMPLETE, SA_AGGLO_AVERAGE
_AGGLO_NAMES = {"complete": AGGLO_COMPLETE, "average": AGGLO_AVERAGE}


def _agglo_method(method) -> int:
    """"complete" / "average" or a number; which numbers are valid is the library's to say"""
    if isinstance(method, str):
        if method not in _AGGLO_NAMES:
            raise AlignError(f"linkage method {method!r} is neither 'complete' nor 'average' (single linkage: hip_linkage)")
        return _AGGLO_NAMES[method]
    m = int(method)
    if not -2**31 <= m < 2**31:
        raise AlignError(f"method = {m} is not an int32")
    return m


def _agglo_quantity(norm: Optional[Norm], pid: Optional[int], n: int):
    """the norm / pid_denom arguments of sa_hip_agglomerate* (both may be given: the library refuses that) and what the
    result gains behind the plain tuple: the n denominators for a norm"""
    cn, den = norm._as_c(n) if norm is not None else (None, None)
    return (C.byref(cn) if cn is not None else None, C.byref(C.c_int32(_denom(pid))) if pid is not None else None,
            (den[:n],) if den is not None else ())


def hip_agglomerate(store: SequenceStore, scoring: Scoring, method, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_agglomerate: the complete-linkage ("complete", 1) or average-linkage / UPGMA ("average", 2) tree, built on the
    device -- (pairs int32 (N - 1, 2) with lo < hi, score int32 (N - 1,)) in the order the merges are made; a cluster is
    named by its smallest member, score is the minimum over the merged clusters' cross pairs, or the floor of their average.
    The matrix never leaves the device.  With a norm: (pairs, score, denominators)."""
    sc, m = scoring._as_c(), _agglo_method(method)
    cn, cd, den = _agglo_quantity(norm, pid, store.num)
    lib = load_library()
    return _take_linkage(lib, lib.sa_hip_agglomerate(store._as_c(), C.byref(sc), m, cn, cd)) + den


def hip_agglomerate_with_ranks(store: SequenceStore, scoring: Scoring, method, ranks, norm: Optional[Norm] = None, pid: Optional[int] = None):
    """sa_hip_agglomerate_with_ranks: one alignment, then hip_select's (values, below) for `ranks` and hip_agglomerate's
    (pairs, score) from the same device matrix -- (pairs, score, values, below); with a norm the denominators follow"""
    sc, m = scoring._as_c(), _agglo_method(method)
    r = _ranks(ranks)
    value, below = _select_room(len(r))
    cn, cd, den = _agglo_quantity(norm, pid, store.num)
    lib = load_library()
    tree = _take_linkage(lib, lib.sa_hip_agglomerate_with_ranks(store._as_c(), C.byref(sc), m, cn, cd, r.ctypes.data, len(r),
                                                                value.ctypes.data, below.ctypes.data))
    return tree + (value[:len(r)].copy(), below[:len(r)].copy()) + den


def agglo_scratch_bytes(n: int, method) -> int:
    """sa_agglo_scratch_bytes: the device scratch memory Context.agglomerate needs for n sequences (0: a bad method or n)"""
    return int(load_library().sa_agglo_scratch_bytes(int(n), _agglo_method(method)))


def last_agglomerate_seconds() -> float:
    """device time of the last hip_agglomerate* / DeflateJob.agglomerate call"""
    return float(load_library().sa_hip_last_agglomerate_seconds())


def last_agglomerate_rescans() -> int:
    """the rows the last hip_agglomerate* / DeflateJob.agglomerate call scanned again after a merge took their cached partner"""
    return int(load_library().sa_hip_last_agglomerate_rescans())


def agglo_labels(pairs, score, n: int, min_score: int) -> tuple[np.ndarray, int]:
    """sa_agglo_labels (host only): (labels int32 (N,), clusters) after the merges with score >= min_score -- labels[r] is the
    smallest index in r's cluster.  For a complete-linkage tree every pair inside a cluster scores at least min_score."""
    n, pairs, score = _tree_arrays(pairs, score, n)
    labels = np.empty(n, np.int32)
    clusters = load_library().sa_agglo_labels(pairs.ctypes.data, score.ctypes.data, n, _min_score(min_score), labels.ctypes.data)
    if clusters < 0:
        raise AlignError(_err())
    return labels, int(clusters)


def linkage_merges(pairs, n: int) -> np.ndarray:
    """sa_linkage_merges (host only): int32 (N - 1, 3), rows (left, right, size) in the convention of scipy.cluster.hierarchy:
    ids below N are sequences, id N + u is the cluster made by merge u"""
    n, pairs, _ = _tree_arrays(pairs, None, n)
    out = np.empty((3, max(n - 1, 1)), np.int32)
    if load_library().sa_linkage_merges(pairs.ctypes.data, n, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data):
        raise AlignError(_err())
    return np.ascontiguousarray(out[:, :n - 1].T)


#: struct sa_aln
ALN_DTYPE = np.dtype([("score", "<i4"), ("a_begin", "<i4"), ("a_end", "<i4"), ("b_begin", "<i4"), ("b_end", "<i4"),
                      ("columns", "<i4"), ("identities", "<i4"), ("cigar_len", "<i4"), ("cigar_off", "<i8")])
CIGAR_OPS = "MID"  # SA_ALN_M: a residue of each, SA_ALN_I: of a only, SA_ALN_D: of b only


@dataclass
class Alignments:
    """What sa_ctx_alignments / sa_hip_alignments return: one record per pair, in the caller's order, and the flat
    run-length CIGARs (uint32 runs, len << 4 | op; record t owns cigar[cigar_off : cigar_off + cigar_len])."""
    pairs: np.ndarray    # int32 [P, 2] = (a, b)
    records: np.ndarray  # ALN_DTYPE [P]
    cigar: np.ndarray    # uint32, flat

    def runs(self, t: int) -> list[tuple[int, str]]:
        r = self.records[t]
        return [(int(w) >> 4, CIGAR_OPS[int(w) & 15]) for w in self.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])]]

    def cigar_string(self, t: int) -> str:
        """e.g. "37M2D61M" ("" for the empty alignment of a Smith-Waterman pair whose best score is 0)"""
        return "".join(f"{n}{op}" for n, op in self.runs(t))

    def aligned(self, t: int, store: "SequenceStore") -> tuple[str, str]:
        """the two gapped strings of pair t: the covered residues of a and of b, '-' where the other sequence has one alone"""
        r = self.records[t]
        sa, sb = store.sequence(int(self.pairs[t, 0])).decode(), store.sequence(int(self.pairs[t, 1])).decode()
        i, j, ga, gb = int(r["a_begin"]), int(r["b_begin"]), [], []
        for n, op in self.runs(t):
            ga.append(sa[i:i + n] if op != "D" else "-" * n)
            gb.append(sb[j:j + n] if op != "I" else "-" * n)
            i += n if op != "D" else 0
            j += n if op != "I" else 0
        return "".join(ga), "".join(gb)


def _pairs_array(pairs) -> np.ndarray:
    arr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), np.int64)
    if arr.size and (arr.min() < -2**31 or arr.max() >= 2**31):
        raise AlignError("pair indices must be int32")
    return np.ascontiguousarray(arr.astype(np.int32))


def _take_alignments(lib, handle, pairs: np.ndarray) -> Alignments:
    if not handle:
        raise AlignError(_err())
    try:
        n = int(lib.sa_alns_count(handle))
        runs = C.c_int64(0)
        cig = lib.sa_alns_cigar(handle, C.byref(runs))
        rec = lib.sa_alns_records(handle)
        records = np.frombuffer(C.string_at(rec, n * ALN_DTYPE.itemsize), dtype=ALN_DTYPE).copy() if n else np.zeros(0, ALN_DTYPE)
        cigar = np.frombuffer(C.string_at(cig, 4 * runs.value), dtype=np.uint32).copy() if runs.value else np.zeros(0, np.uint32)
    finally:
        lib.sa_alns_destroy(handle)
    return Alignments(pairs=pairs, records=records, cigar=cigar)


def hip_alignments(store: SequenceStore, scoring: Scoring, pairs) -> Alignments:
    """sa_hip_alignments: the alignments of the listed pairs (a, b), a != b, any order, duplicates allowed -- traced back
    on the device.  The contract (orientation, tie rule, what a CIGAR scores) is in include/seqalign_hip.h."""
    lib = load_library()
    arr = _pairs_array(pairs)
    a, b = np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1])
    sc = scoring._as_c()
    return _take_alignments(lib, lib.sa_hip_alignments(store._as_c(), C.byref(sc), a.ctypes.data, b.ctypes.data, len(arr)), arr)


def last_alignments_seconds() -> float:
    """device time (fill + walk) of the last hip_alignments / Context.alignments call"""
    return float(load_library().sa_hip_last_alignments_seconds())


def last_alignments_breakdown() -> dict:
    """... and its parts: fill_seconds, walk_seconds, the DP cells filled and the number of batches"""
    f, w, c, b = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int32(0)
    load_library().sa_hip_last_alignments_breakdown(C.byref(f), C.byref(w), C.byref(c), C.byref(b))
    return {"fill_seconds": f.value, "walk_seconds": w.value, "cells": c.value, "batches": b.value}


class PinnedMatrix:
    """A host result matrix page-locked once (what a C host does in output_load with sa_hip_host_register), so that
    repeated deliveries into it are pure DMA / direct stores.  `.array` is the flat int32 numpy view.

    `shared=path`: the matrix is a shared file mapping (e.g. under /dev/shm) that every rank of a node attaches and
    page-locks -- one host matrix for a one-process-per-GPU run, the reference's single mmap-ed result
    (src/io/output.c:55) -- created by the rank that passes create=True, zero-filled."""

    def __init__(self, elements: int, shared: Optional[str] = None, create: bool = True):
        self._lib = load_library()
        if shared is not None:
            if create:
                with open(shared, "wb") as f:
                    f.truncate(4 * max(int(elements), 1))
            self.array = np.memmap(shared, dtype=np.int32, mode="r+", shape=(max(int(elements), 1),))[:int(elements)]
        else:
            # an anonymous mapping of its own, never malloc's heap: the library refuses to page-lock memory that malloc hands
            # out again, and a C host's matrix is a mapping anyway (output_load, src/io/output.c:55)
            import mmap
            self._map = mmap.mmap(-1, 4 * max(int(elements), 1))
            self.array = np.frombuffer(self._map, dtype=np.int32)[:int(elements)]
        self.path = shared
        self._registered = False
        if elements and self._lib.sa_hip_host_register(C.c_void_p(self.array.ctypes.data), self.array.nbytes):
            raise AlignError(_err())
        self._registered = bool(elements)

    @property
    def ptr(self) -> int:
        return int(self.array.ctypes.data)

    def close(self) -> None:
        if self._registered:
            self._registered = False
            try:
                self._lib.sa_hip_host_unregister(C.c_void_p(self.array.ctypes.data))
            except ImportError:  # interpreter shutting down: the process's mappings go with it
                pass

    __del__ = close


def hip_filter(store: SequenceStore, threshold: float) -> np.ndarray:
    """`filter()` replacement (reference src/bio/filter.c:14-89): boolean keep mask with the sequential semantics
    of `-f threshold`; the similarity relation is computed on the device."""
    keep = np.ones(store.num, dtype=np.uint8)
    rc = load_library().sa_hip_filter(store._as_c(), C.c_float(threshold), keep.ctypes.data)
    if rc < 0:
        raise AlignError(_err())
    return keep.astype(bool)


class Context:
    """Device-resident layer (sa_ctx_*): sequences + scoring uploaded once, ranges of the packed pair
    index computed into device buffers the caller owns (e.g. torch tensors)."""

    def __init__(self, store: SequenceStore, scoring: Scoring, device: int = 0):
        sc = scoring._as_c()
        self._adopt(lambda lib: lib.sa_ctx_create(int(device), store._as_c(), C.byref(sc)), store, store.num, device)

    def _adopt(self, create, keep, num: int, device: int) -> None:
        """the state every context has, whichever call creates it: the library, the handle of create(lib), what keeps the
        host arrays alive, the number of sequences in the context's store, the device"""
        self._lib = load_library()
        self._store = keep
        self._h = create(self._lib)
        if not self._h:
            raise AlignError(_err())
        self.num = int(num)
        self.device = int(device)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.sa_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def pairs(self) -> int:
        return int(self._lib.sa_ctx_pairs(self._h))

    def cells(self, start: int = 0, count: Optional[int] = None) -> int:
        return self._store.cells(start, count)

    def partition(self, parts: int) -> list[int]:
        return self._store.partition(parts)

    def align_range(self, start: int, count: int, d_scores_ptr: int, stream: int = 0) -> None:
        if self._lib.sa_ctx_align_range(self._h, start, count, C.c_void_p(d_scores_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def token_tiles(self) -> tuple[int, int]:
        """packed tiles of the last launch as (lean, legacy): streaming the token streams built beside the arranged copies /
        deriving their tokens from the code bytes in the kernel (partial and store-order tiles, SA_HIP_NO_TOKENS=1)"""
        lean, legacy = C.c_int64(0), C.c_int64(0)
        if self._lib.sa_ctx_token_tiles(self._h, C.byref(lean), C.byref(legacy)):
            raise AlignError(_err())
        return int(lean.value), int(legacy.value)

    @property
    def scores_fit16(self) -> bool:
        """every score of this store under this scoring provably fits int16 (exchange format of the all-gather)"""
        return bool(self._lib.sa_ctx_scores_fit16(self._h))

    def align_range16(self, start: int, count: int, d_scores16_ptr: int, stream: int = 0) -> None:
        """as align_range, into an int16 device array; raises when scores_fit16 is False"""
        if self._lib.sa_ctx_align_range16(self._h, start, count, C.c_void_p(d_scores16_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def widen16(self, d_src16_ptr: int, d_dst32_ptr: int, count: int, stream: int = 0) -> None:
        """int16 exchange format -> the reference's s32, on the device"""
        if self._lib.sa_hip_widen16(C.c_void_p(d_src16_ptr), C.c_void_p(d_dst32_ptr), count, C.c_void_p(stream)):
            raise AlignError(_err())

    # ---- tile-interleaved sharding (one process per GPU; sequencealigner_amd/distributed.py: TiledGatherStep) ----
    def leave_room(self, on: bool) -> None:
        """three instead of four persistent workgroups per CU from now on: room for a concurrent collective / placement"""
        self._lib.sa_ctx_leave_room(self._h, int(on))

    def share_elems(self, start: int, count: int, world: int, to_host: bool = False) -> int:
        """elements of one rank's dense share of the packed range (the same on every rank)"""
        v = int(self._lib.sa_ctx_share_elems(self._h, start, count, world, int(to_host)))
        if v < 0:
            raise AlignError(_err())
        return v

    def align_share(self, start: int, count: int, world: int, rank: int, d_share_ptr: int, elem16: bool, stream: int = 0,
                    host_packed_ptr: int = 0) -> None:
        """scores of `rank`'s tiles of the range, densely in tile order (int16 or s32 elements); with host_packed_ptr (the
        WHOLE page-locked packed host matrix) the same scores also go straight to host_packed[p]"""
        if self._lib.sa_ctx_align_share(self._h, start, count, world, rank, C.c_void_p(d_share_ptr), int(elem16),
                                        C.c_void_p(host_packed_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def place_shares(self, start: int, count: int, world: int, d_shares_ptr: int, elem16: bool, d_packed_ptr: int, stream: int = 0,
                     to_host: bool = False) -> None:
        """gathered shares (rank-major) -> d_packed[p - start], the reference's packed order, widened to s32"""
        if self._lib.sa_ctx_place_shares(self._h, start, count, world, int(to_host), C.c_void_p(d_shares_ptr), int(elem16),
                                         C.c_void_p(d_packed_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def align_host(self, matrix: Optional[np.ndarray], triangular: bool, start: int = 0, count: Optional[int] = None) -> float:
        """The reference's launch/copy loop (seqalign_cuda.c:182-292) on this context: scores of the packed range into
        the host matrix (a flat int32 array: packed N(N-1)/2 or full N*N; None = the reference's -W).  Returns the
        seconds the loop took (uploads, allocations and page-locking are outside it, as in the reference)."""
        count = self.pairs - start if count is None else count
        out = _Output(matrix.ctypes.data if matrix is not None else None, None, self.num, bool(triangular))
        phase = C.c_double()
        if self._lib.sa_ctx_align_host(self._h, start, count, out, C.byref(phase)):
            raise AlignError(_err())
        return float(phase.value)

    def expand_full(self, d_packed_ptr: int, d_full_ptr: int, stream: int = 0) -> None:
        if self._lib.sa_ctx_expand_full(self._h, C.c_void_p(d_packed_ptr), C.c_void_p(d_full_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def neighbors(self, d_packed_ptr: int, k: int, d_index_ptr: int, d_score_ptr: int, stream: int = 0) -> None:
        """sa_ctx_neighbors: from the whole packed device matrix of this store, the k best partners of every sequence into
        the device arrays d_index / d_score (N * k int32 each), asynchronously on `stream`"""
        if self._lib.sa_ctx_neighbors(self._h, C.c_void_p(d_packed_ptr), int(k), C.c_void_p(d_index_ptr), C.c_void_p(d_score_ptr),
                                      C.c_void_p(stream)):
            raise AlignError(_err())

    def edge_offsets(self, d_packed_ptr: int, min_score: int, d_offsets_ptr: int, stream: int = 0) -> None:
        """sa_ctx_edge_offsets: from the whole packed device matrix of this store, the CSR offsets (N + 1 int64, device memory)
        of the pairs that score at least min_score, asynchronously on `stream`; offsets[N] = E"""
        if self._lib.sa_ctx_edge_offsets(self._h, C.c_void_p(d_packed_ptr), _min_score(min_score), C.c_void_p(d_offsets_ptr),
                                         C.c_void_p(stream)):
            raise AlignError(_err())

    def edge_fill(self, d_packed_ptr: int, min_score: int, d_offsets_ptr: int, d_index_ptr: int, d_score_ptr: int, stream: int = 0) -> None:
        """sa_ctx_edge_fill: with the offsets edge_offsets wrote for the same matrix and threshold, the columns (ascending per
        row) and scores into the device arrays d_index / d_score (E int32 each), asynchronously on `stream`"""
        if self._lib.sa_ctx_edge_fill(self._h, C.c_void_p(d_packed_ptr), _min_score(min_score), C.c_void_p(d_offsets_ptr),
                                      C.c_void_p(d_index_ptr), C.c_void_p(d_score_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def linkage(self, d_packed_ptr: int, d_pairs_ptr: int, d_score_ptr: int, d_scratch_ptr: int, stream: int = 0) -> None:
        """sa_ctx_linkage: from the whole packed device matrix of this store, the single-linkage tree into the device arrays
        d_pairs (2 (N - 1) int32) / d_score (N - 1 int32), asynchronously on `stream`; d_scratch: linkage_scratch_bytes(N) bytes"""
        if self._lib.sa_ctx_linkage(self._h, C.c_void_p(d_packed_ptr), C.c_void_p(d_pairs_ptr), C.c_void_p(d_score_ptr),
                                    C.c_void_p(d_scratch_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def agglomerate(self, d_packed_ptr: int, method, d_pairs_ptr: int, d_score_ptr: int, d_scratch_ptr: int, stream: int = 0) -> None:
        """sa_ctx_agglomerate: from the whole packed device matrix of this store, the complete- or average-linkage tree into the
        device arrays d_pairs (2 (N - 1) int32) / d_score (N - 1 int32), asynchronously on `stream`; d_scratch:
        agglo_scratch_bytes(N, method) bytes, 8-byte aligned, contents ignored"""
        if self._lib.sa_ctx_agglomerate(self._h, C.c_void_p(d_packed_ptr), _agglo_method(method), C.c_void_p(d_pairs_ptr),
                                        C.c_void_p(d_score_ptr), C.c_void_p(d_scratch_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def select(self, d_packed_ptr: int, ranks, d_value_ptr: int, d_below_ptr: int, d_scratch_ptr: int, stream: int = 0) -> None:
        """sa_ctx_select: from the whole packed device matrix of this store (any 4-byte-aligned device pointer), the scores at
        `ranks` (host values, up to 16) into d_value (m int32) and the pairs below each into d_below (m int64), asynchronously on
        `stream`; d_scratch: select_scratch_bytes(m) bytes, 8-byte aligned, contents ignored"""
        r = _ranks(ranks)
        if self._lib.sa_ctx_select(self._h, C.c_void_p(d_packed_ptr), r.ctypes.data, len(r), C.c_void_p(d_value_ptr),
                                   C.c_void_p(d_below_ptr), C.c_void_p(d_scratch_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def denominators(self, source: int, d_den_ptr: int, stream: int = 0) -> None:
        """sa_ctx_denominators: the per-sequence denominators (NORM_SELF: self-scores by the full DP, NORM_LENGTH: lengths) into
        the device array d_den (N int32), asynchronously on `stream`; not beside align_range of this context on another stream"""
        source = int(source)
        if not -2**31 <= source < 2**31:
            raise AlignError(f"source = {source} is not an int32")
        if self._lib.sa_ctx_denominators(self._h, source, C.c_void_p(d_den_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def normalize(self, d_packed_ptr: int, d_den_ptr: int, rule: int, d_out_ptr: int, stream: int = 0) -> None:
        """sa_ctx_normalize: the whole packed device matrix of this store divided by the denominators d_den (any N int32 of
        device memory) under `rule`, into d_out -- d_packed itself (in place) or a disjoint buffer -- asynchronously on `stream`"""
        rule = int(rule)
        if not -2**31 <= rule < 2**31:
            raise AlignError(f"rule = {rule} is not an int32")
        if self._lib.sa_ctx_normalize(self._h, C.c_void_p(d_packed_ptr or None), C.c_void_p(d_den_ptr or None), rule,
                                      C.c_void_p(d_out_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def identity_range(self, start: int, count: int, score: int = 0, identities: int = 0, columns: int = 0, pid: int = 0,
                       denom: int = 0, stream: int = 0) -> None:
        """sa_ctx_identity_range: score / identities / columns / pid of the packed pair range [start, start + count) into the
        device arrays given (count int32 each, 0: not asked for; `denom` is read iff pid), asynchronously on `stream`; not beside
        align_range or another identity_range of this context on another stream"""
        out = _IdentityOut(score or None, identities or None, columns or None, pid or None, _denom(denom))
        if self._lib.sa_ctx_identity_range(self._h, int(start), int(count), C.byref(out), C.c_void_p(stream)):
            raise AlignError(_err())

    def alignments(self, pairs) -> Alignments:
        """sa_ctx_alignments: the alignments of the listed pairs of this context's store (see hip_alignments)"""
        arr = _pairs_array(pairs)
        a, b = np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1])
        return _take_alignments(self._lib, self._lib.sa_ctx_alignments(self._h, a.ctypes.data, b.ctypes.data, len(arr)), arr)

    def timing(self, enable: bool) -> None:
        self._lib.sa_ctx_timing(self._h, int(enable))

    def timing_read(self) -> dict:
        """Dominant kernel since timing(True): name, launches, total ms, pairs and cells it covered."""
        name = C.create_string_buffer(256)
        launches, pairs, cells = C.c_int64(), C.c_int64(), C.c_int64()
        ms, all_ms = C.c_double(), C.c_double()
        if self._lib.sa_ctx_timing_read(self._h, name, 256, C.byref(launches), C.byref(ms), C.byref(pairs),
                                        C.byref(cells), C.byref(all_ms)):
            raise AlignError(_err())
        return dict(kernel=name.value.decode(), launches=int(launches.value), ms=float(ms.value),
                    pairs=int(pairs.value), cells=int(cells.value), all_kernels_ms=float(all_ms.value))


def _int32(name: str, v) -> int:
    v = int(v)
    if not -2**31 <= v < 2**31:
        raise AlignError(f"{name} = {v} is not an int32")
    return v


class SearchContext(Context):
    """Search context (sa_ctx_create_search): db followed by queries as one store whose launches are bounded to the database
    rows.  search_range computes the (nq, N) rectangle of a query range into device memory, hits selects the k best database
    sequences of every row; alignments takes pairs (N + q, d).  The packed-range calls inherited from Context are refused by the
    library on such a context."""

    def __init__(self, db: SequenceStore, queries: SequenceStore, scoring: Scoring, device: int = 0, strands: bool = False,
                 comp: Optional[np.ndarray] = None):
        """strands=True: a strands context (sa_ctx_create_search_strands) -- the query rows are the M queries followed by their M
        reverse complements under `comp` (128 uint8; None: dna_complement()), n_queries answers 2 M and n_strand_queries M"""
        sc = scoring._as_c()
        if strands:
            table = None if comp is None else _comp_table(comp)
            self._adopt(lambda lib: lib.sa_ctx_create_search_strands(int(device), db._as_c(), queries._as_c(), C.byref(sc),
                                                                     None if table is None else table.ctypes.data),
                        (db, queries), db.num + 2 * queries.num, device)
        else:
            self._adopt(lambda lib: lib.sa_ctx_create_search(int(device), db._as_c(), queries._as_c(), C.byref(sc)), (db, queries),
                        db.num + queries.num, device)
        self.n_db = int(self._lib.sa_ctx_search_db(self._h))
        self.n_queries = int(self._lib.sa_ctx_search_queries(self._h))
        self.strands = int(self._lib.sa_ctx_search_strands(self._h))
        self.n_strand_queries = self.n_queries // 2 if self.strands == 2 else self.n_queries

    def strand_fold(self, d_vfwd_ptr: int, d_vrev_ptr: int, nq: int, d_vbest_ptr: int, d_bits_ptr: int = 0, d_sfwd_ptr: int = 0,
                    d_srev_ptr: int = 0, d_sbest_ptr: int = 0, stream: int = 0) -> None:
        """sa_ctx_strand_fold: rows [0, nq) at pitch N of the value rectangles of the two strands folded into d_vbest (the larger
        value; the forward one on a tie), the raw scores d_sfwd / d_srev carried along into d_sbest (all three or none), the strand
        of every cell into the bitmap d_bits (nq * strand_words(N) uint64, 8-byte aligned; 0: not asked for).  d_vbest may be
        d_vfwd and d_sbest may be d_sfwd."""
        if self._lib.sa_ctx_strand_fold(self._h, C.c_void_p(d_vfwd_ptr or None), C.c_void_p(d_vrev_ptr or None), C.c_void_p(d_sfwd_ptr or None),
                                        C.c_void_p(d_srev_ptr or None), _int32("nq", nq), C.c_void_p(d_vbest_ptr or None),
                                        C.c_void_p(d_sbest_ptr or None), C.c_void_p(d_bits_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def hits_strand(self, d_bits_ptr: int, nq: int, k: int, d_index_ptr: int, d_strand_ptr: int, stream: int = 0) -> None:
        """sa_ctx_hits_strand: d_strand[r, t] (uint8) = the strand of cell (r, d_index[r, t]) for rows [0, nq) of an (nq, k) hit
        list; STRAND_NONE for an index outside [0, N)"""
        if self._lib.sa_ctx_hits_strand(self._h, C.c_void_p(d_bits_ptr or None), _int32("nq", nq), _int32("k", k), C.c_void_p(d_index_ptr or None),
                                        C.c_void_p(d_strand_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def hits_above_strand(self, d_bits_ptr: int, nq: int, d_offsets_ptr: int, d_index_ptr: int, d_strand_ptr: int, stream: int = 0) -> None:
        """sa_ctx_hits_above_strand: the strand (uint8) of every entry of a CSR over rows [0, nq): row r owns entries
        offsets[r] .. offsets[r + 1] (int64) of d_index / d_strand"""
        if self._lib.sa_ctx_hits_above_strand(self._h, C.c_void_p(d_bits_ptr or None), _int32("nq", nq), C.c_void_p(d_offsets_ptr or None),
                                              C.c_void_p(d_index_ptr or None), C.c_void_p(d_strand_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def cells(self, start: int = 0, count: Optional[int] = None) -> int:
        raise AlignError("a search context has no packed pair space")

    def partition(self, parts: int) -> list[int]:
        raise AlignError("a search context has no packed pair space")

    def search_scratch_bytes(self, q0: int, nq: int) -> int:
        return int(self._lib.sa_search_scratch_bytes(self._h, _int32("q0", q0), _int32("nq", nq)))

    def search_range(self, q0: int, nq: int, d_rect_ptr: int, d_scratch_ptr: int, stream: int = 0) -> None:
        """sa_ctx_search_range: queries [q0, q0 + nq) into the dense device rectangle d_rect[(q - q0) * N + d]"""
        if self._lib.sa_ctx_search_range(self._h, _int32("q0", q0), _int32("nq", nq), C.c_void_p(d_rect_ptr), C.c_void_p(d_scratch_ptr),
                                         C.c_void_p(stream)):
            raise AlignError(_err())

    def hits(self, d_rect_ptr: int, nq: int, k: int, d_index_ptr: int, d_score_ptr: int, d_scratch_ptr: int = 0, stream: int = 0) -> None:
        """sa_ctx_hits: the k best database sequences of rows [0, nq) of a device rectangle of pitch N"""
        if self._lib.sa_ctx_hits(self._h, C.c_void_p(d_rect_ptr), _int32("nq", nq), _int32("k", k), C.c_void_p(d_index_ptr),
                                 C.c_void_p(d_score_ptr), C.c_void_p(d_scratch_ptr), C.c_void_p(stream)):
            raise AlignError(_err())

    def normalize_rect(self, d_rect_ptr: int, nq: int, q0: int, d_den_ptr: int, rule: int, d_out_ptr: int, stream: int = 0) -> None:
        """sa_ctx_normalize_rect: rows [0, nq) of a device rectangle of pitch N whose row r is query q0 + r, divided by the
        denominators d_den (N + M int32 of device memory: denominators() of this context, or the caller's own) under `rule`, into
        d_out -- d_rect itself (in place) or a disjoint buffer -- asynchronously on `stream`"""
        if self._lib.sa_ctx_normalize_rect(self._h, C.c_void_p(d_rect_ptr or None), _int32("nq", nq), _int32("q0", q0),
                                           C.c_void_p(d_den_ptr or None), _int32("rule", rule), C.c_void_p(d_out_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def identity_rect(self, q0: int, nq: int, score: int = 0, identities: int = 0, columns: int = 0, pid: int = 0, denom: int = 0,
                      stream: int = 0) -> None:
        """sa_ctx_identity_rect: score / identities / columns / pid of queries [q0, q0 + nq) against every database sequence into
        the device arrays given (nq * N int32 each, element (q - q0) * N + d; 0: not asked for; `denom` is read iff pid),
        asynchronously on `stream`; not beside another sweep of this context on another stream"""
        out = _IdentityOut(score or None, identities or None, columns or None, pid or None, _denom(denom))
        if self._lib.sa_ctx_identity_rect(self._h, _int32("q0", q0), _int32("nq", nq), C.byref(out), C.c_void_p(stream)):
            raise AlignError(_err())

    def fit_rect(self, q0: int, nq: int, score: int = 0, db_begin: int = 0, db_end: int = 0, identities: int = 0, columns: int = 0, pid: int = 0,
                 denom: int = 0, stream: int = 0) -> None:
        """sa_ctx_fit_rect: queries [q0, q0 + nq) fitted inside every database sequence -- the whole query, the database's overhang
        free -- into the device arrays given (nq * N int32 each, element (q - q0) * N + d; 0: not asked for; `denom` is read iff pid),
        asynchronously on `stream`; not beside another sweep of this context on another stream.  NW and Gotoh contexts only."""
        out = _FitOut(score or None, db_begin or None, db_end or None, identities or None, columns or None, pid or None, _denom(denom))
        if self._lib.sa_ctx_fit_rect(self._h, _int32("q0", q0), _int32("nq", nq), C.byref(out), C.c_void_p(stream)):
            raise AlignError(_err())

    def fit_pairs(self, d_query_ptr: int, d_db_ptr: int, npairs: int, score: int = 0, db_begin: int = 0, db_end: int = 0, identities: int = 0,
                  columns: int = 0, pid: int = 0, denom: int = 0, stream: int = 0) -> None:
        """sa_ctx_fit_pairs: the list form of fit_rect -- item w is query d_query[w] against database sequence d_db[w] (device int32
        arrays, read in stream order), element w of every output given; an index out of range gives INT32_MIN"""
        out = _FitOut(score or None, db_begin or None, db_end or None, identities or None, columns or None, pid or None, _denom(denom))
        if self._lib.sa_ctx_fit_pairs(self._h, C.c_void_p(d_query_ptr or None), C.c_void_p(d_db_ptr or None), C.c_int64(int(npairs)), C.byref(out),
                                      C.c_void_p(stream)):
            raise AlignError(_err())

    def fit_alignments(self, pairs) -> Alignments:
        """sa_ctx_fit_alignments: the fitted alignments of the listed pairs (query, database sequence) -- query in [0, n_queries),
        database sequence in [0, n_db), any order, duplicates allowed.  In the records a is the query (a_begin = 0, a_end = its
        length) and b the database sequence (b_begin = db_begin, b_end = db_end); "I" is a residue of the query only.  `pairs` of the
        result holds (query, database sequence) as given."""
        arr = _pairs_array(pairs)
        q, d = np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1])
        return _take_alignments(self._lib, self._lib.sa_ctx_fit_alignments(self._h, q.ctypes.data, d.ctypes.data, len(arr)), arr)

    def hits_take(self, d_rect_ptr: int, nq: int, k: int, d_index_ptr: int, d_out_ptr: int, stream: int = 0) -> None:
        """sa_ctx_hits_take: d_out[r, t] = d_rect[r, d_index[r, t]] for rows [0, nq) -- the raw scores of hits selected on a value
        rectangle"""
        if self._lib.sa_ctx_hits_take(self._h, C.c_void_p(d_rect_ptr or None), _int32("nq", nq), _int32("k", k), C.c_void_p(d_index_ptr or None),
                                      C.c_void_p(d_out_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def hits_above_offsets(self, d_vrect_ptr: int, nq: int, min_value: int, d_offsets_ptr: int, d_scratch_ptr: int, stream: int = 0) -> None:
        """sa_ctx_hits_above_offsets: count + scan -- the nq + 1 int64 CSR offsets of the hits (value >= min_value) of rows [0, nq)
        of a device rectangle of pitch N; d_scratch: hits_above_scratch_bytes(N, nq) bytes, 8-byte aligned, kept for the fill"""
        if self._lib.sa_ctx_hits_above_offsets(self._h, C.c_void_p(d_vrect_ptr or None), _int32("nq", nq), _int32("min_value", min_value),
                                               C.c_void_p(d_offsets_ptr or None), C.c_void_p(d_scratch_ptr or None), C.c_void_p(stream)):
            raise AlignError(_err())

    def hits_above_fill(self, d_vrect_ptr: int, d_rect_ptr: int, nq: int, min_value: int, d_offsets_ptr: int, d_scratch_ptr: int,
                        d_index_ptr: int, d_value_ptr: int = 0, d_score_ptr: int = 0, stream: int = 0) -> None:
        """sa_ctx_hits_above_fill: index (ascending d per row), value and raw score of every hit, E = offsets[nq] int32 each, from
        the offsets and scratch hits_above_offsets left for the same rectangle, nq and min_value; d_value / d_score 0: not asked
        for; d_rect is read iff d_score"""
        if self._lib.sa_ctx_hits_above_fill(self._h, C.c_void_p(d_vrect_ptr or None), C.c_void_p(d_rect_ptr or None), _int32("nq", nq),
                                            _int32("min_value", min_value), C.c_void_p(d_offsets_ptr or None), C.c_void_p(d_scratch_ptr or None),
                                            C.c_void_p(d_index_ptr or None), C.c_void_p(d_value_ptr or None), C.c_void_p(d_score_ptr or None),
                                            C.c_void_p(stream)):
            raise AlignError(_err())


def hits_above_scratch_bytes(n_db: int, nq: int) -> int:
    """device bytes SearchContext.hits_above_offsets / _fill need as scratch: 8 * (nq * S + 1), S the segments of a row"""
    return int(load_library().sa_hits_above_scratch_bytes(_int32("n_db", n_db), _int32("nq", nq)))


def hits_scratch_bytes(n_db: int, nq: int, k: int) -> int:
    """device bytes SearchContext.hits needs as scratch (0: none, the rows alone fill the device)"""
    return int(load_library().sa_hits_scratch_bytes(_int32("n_db", n_db), _int32("nq", nq), _int32("k", k)))


def _search_quantity(db: SequenceStore, queries: SequenceStore, scoring: Scoring, k: Optional[int], rect: bool, norm: Optional["Norm"],
                     pid: Optional[int]):
    """sa_hip_search_norm / sa_hip_search_pid: (index, value, score[, rect, vrect][, denominators])"""
    n, m = db.num, queries.num
    if k is None and not rect:
        raise AlignError("hip_search: nothing asked for (k is None and rect is False)")
    kk = 0 if k is None else _int32("k", k)
    index = value = score = out = vout = None
    if k is not None:
        rows = max(m, 1) * max(min(kk, NEIGHBORS_MAX), 1)
        index, value, score = (np.empty(rows, np.int32) for _ in range(3))
    if rect:
        out, vout = np.empty((max(m, 0), max(n, 0)), np.int32), np.empty((max(m, 0), max(n, 0)), np.int32)
    ptr = [None if a is None else a.ctypes.data for a in (index, value, score, out, vout)]
    sc = scoring._as_c()
    lib = load_library()
    tail = ()
    if norm is not None:
        cn, den = norm._as_c(n + m)
        ok = lib.sa_hip_search_norm(db._as_c(), queries._as_c(), C.byref(sc), kk, *ptr, C.byref(cn))
        tail = (den[:n + m],)
    elif pid is not None:
        ok = lib.sa_hip_search_pid(db._as_c(), queries._as_c(), C.byref(sc), kk, *ptr, _denom(pid))
    else:  # (values=True without a quantity: norm == NULL, value a copy of score)
        ok = lib.sa_hip_search_norm(db._as_c(), queries._as_c(), C.byref(sc), kk, *ptr, None)
    if not ok:
        raise AlignError(_err())
    res = ()
    if k is not None:
        res += tuple(a[:m * kk].reshape(m, kk) for a in (index, value, score))
    if rect:
        res += (out, vout)
    return res + tail


def hip_search(db: SequenceStore, queries: SequenceStore, scoring: Scoring, k: Optional[int] = None, rect: bool = False,
               norm: Optional["Norm"] = None, pid: Optional[int] = None, values: bool = False):
    """sa_hip_search: queries against a database on the first device.  With k: (index, score), two (M, k) int32 arrays, row q
    lists the database sequences by score descending, then index ascending; 1 <= k <= min(N, NEIGHBORS_MAX).  With rect=True
    the (M, N) int32 rectangle rect[q, d] follows (alone when k is None).

    With a quantity -- norm=Norm(source, rule): normalised scores, or pid=PID_*: percent identity, both in parts per million
    (sa_hip_search_norm / sa_hip_search_pid) -- or with values=True the hits are ranked by the value and the result is
    (index, value, score[, rect, vrect]): value descending, then index ascending; score is the raw score of each hit, not sorted;
    vrect the (M, N) values.  A norm appends the N + M denominators (database first).  values=True without a quantity gives value
    = score and vrect = rect.  Asking for both quantities is a ValueError."""
    if norm is not None and pid is not None:
        raise ValueError("hip_search: norm and pid exclude each other")
    if norm is not None or pid is not None or values:
        return _search_quantity(db, queries, scoring, k, rect, norm, pid)
    n, m = db.num, queries.num
    if k is None and not rect:
        raise AlignError("hip_search: nothing asked for (k is None and rect is False)")
    kk = 0 if k is None else _int32("k", k)
    index = score = out = None
    if k is not None:
        rows = max(m, 1) * max(min(kk, NEIGHBORS_MAX), 1)
        index, score = np.empty(rows, np.int32), np.empty(rows, np.int32)
    if rect:
        out = np.empty((max(m, 0), max(n, 0)), np.int32)
    sc = scoring._as_c()
    if not load_library().sa_hip_search(db._as_c(), queries._as_c(), C.byref(sc), kk, index.ctypes.data if index is not None else None,
                                        score.ctypes.data if score is not None else None, out.ctypes.data if out is not None else None):
        raise AlignError(_err())
    res = ()
    if k is not None:
        res += (index[:m * kk].reshape(m, kk), score[:m * kk].reshape(m, kk))
    if rect:
        res += (out,)
    return res[0] if len(res) == 1 else res


def hip_search_fit(db: SequenceStore, queries: SequenceStore, scoring: Scoring, k: Optional[int] = None, rect: bool = False,
                   pid: Optional[int] = None):
    """sa_hip_search_fit: every query fitted inside every database sequence (the whole query, the database's overhang free; NW or
    Gotoh) on the first device.  With k: (index, value, score, db_begin, db_end), five (M, k) int32 arrays -- row q lists the
    database sequences by value descending, then index ascending; value is the fit score, or with pid=PID_* the percent identity
    of the fitted alignment in parts per million; score is the fit score of each hit and [db_begin, db_end) the span of the
    database sequence the query sits in.  With rect=True the (M, N) rectangles rect (fit scores) and vrect (values) follow (alone
    when k is None)."""
    n, m = db.num, queries.num
    if k is None and not rect:
        raise AlignError("hip_search_fit: nothing asked for (k is None and rect is False)")
    kk = 0 if k is None else _int32("k", k)
    hits = [None] * 5
    out = vout = None
    if k is not None:
        rows = max(m, 1) * max(min(kk, NEIGHBORS_MAX), 1)
        hits = [np.empty(rows, np.int32) for _ in range(5)]
    if rect:
        out, vout = np.empty((max(m, 0), max(n, 0)), np.int32), np.empty((max(m, 0), max(n, 0)), np.int32)
    ptr = [None if a is None else a.ctypes.data for a in (*hits, out, vout)]
    sc = scoring._as_c()
    if not load_library().sa_hip_search_fit(db._as_c(), queries._as_c(), C.byref(sc), kk, -1 if pid is None else _denom(pid), *ptr):
        raise AlignError(_err())
    res = ()
    if k is not None:
        res += tuple(a[:m * kk].reshape(m, kk) for a in hits)
    if rect:
        res += (out, vout)
    return res


def last_search_fit_seconds() -> float:
    """device time of the fit sweeps (rectangle and list) of the last hip_search_fit call, summed over its batches"""
    return float(load_library().sa_hip_last_search_fit_seconds())


class HitList:
    """what hip_search_above returns: the hits of every query as a CSR -- offsets (M + 1, int64), and per hit index (ascending
    within a query), value (the thresholded quantity) and score (the raw score), int32[E]; denominators (N + M) under a norm;
    strand (uint8[E], 0 forward, 1 reverse) from hip_search_above_strands, None otherwise"""

    def __init__(self, offsets: np.ndarray, index: np.ndarray, value: np.ndarray, score: np.ndarray, denominators: Optional[np.ndarray] = None,
                 strand: Optional[np.ndarray] = None):
        self.offsets, self.index, self.value, self.score, self.denominators = offsets, index, value, score, denominators
        self.strand = strand

    def __len__(self) -> int:
        return int(self.index.shape[0])

    def row(self, q: int) -> slice:
        return slice(int(self.offsets[q]), int(self.offsets[q + 1]))


def hip_search_above(db: SequenceStore, queries: SequenceStore, scoring: Scoring, min_value: int, norm: Optional["Norm"] = None,
                     pid: Optional[int] = None) -> HitList:
    """sa_hip_search_above: every database sequence whose value against a query is at least min_value, on the first device.  The
    value is the raw score, or with norm=Norm(source, rule) the normalised score, or with pid=PID_* percent identity, both in
    parts per million.  Any int32 threshold is valid.  Asking for both quantities is the library's to refuse."""
    return _search_above(db, queries, scoring, min_value, norm, pid, False, None)


def hip_search_above_strands(db: SequenceStore, queries: SequenceStore, scoring: Scoring, min_value: int, norm: Optional["Norm"] = None,
                             pid: Optional[int] = None, comp: Optional[np.ndarray] = None) -> HitList:
    """sa_hip_search_above_strands: hip_search_above over the values of both strands of DNA queries, folded on the device; the
    HitList carries strand (0 forward, 1 reverse), and under a norm the N + 2 M denominators"""
    return _search_above(db, queries, scoring, min_value, norm, pid, True, comp)


def _search_above(db, queries, scoring, min_value, norm, pid, strands: bool, comp) -> HitList:
    lib = load_library()
    sc = scoring._as_c()
    t = _int32("min_value", min_value)
    cn = den = None
    dens = db.num + (2 if strands else 1) * queries.num
    if norm is not None:
        cn, den = norm._as_c(dens)
    cd = None if pid is None else C.c_int32(_denom(pid))
    quantity = (None if cn is None else C.byref(cn), None if cd is None else C.byref(cd))
    if strands:
        table = None if comp is None else _comp_table(comp)
        handle = lib.sa_hip_search_above_strands(db._as_c(), queries._as_c(), C.byref(sc), None if table is None else table.ctypes.data, t, *quantity)
    else:
        handle = lib.sa_hip_search_above(db._as_c(), queries._as_c(), C.byref(sc), t, *quantity)
    if not handle:
        raise AlignError(_err())
    try:
        m, count = C.c_int32(0), C.c_int64(0)
        off = lib.sa_hitlist_offsets(handle, C.byref(m))
        ptrs = (lib.sa_hitlist_index(handle, C.byref(count)), lib.sa_hitlist_value(handle), lib.sa_hitlist_score(handle))
        e = count.value
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_int64)), (m.value + 1,)).copy()
        index, value, score = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (e,)).copy() if e else np.zeros(0, np.int32) for p in ptrs)
        strand = None
        sp = lib.sa_hitlist_strand(handle)
        if sp:
            strand = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint8)), (e,)).copy() if e else np.zeros(0, np.uint8)
    finally:
        lib.sa_hitlist_destroy(handle)
    return HitList(offsets, index, value, score, None if den is None else den[:dens], strand)


def last_search_above_seconds() -> float:
    """device time of count + scan + fill in the last hip_search_above call, summed over its batches"""
    return float(load_library().sa_hip_last_search_above_seconds())


STRAND_FORWARD, STRAND_REVERSE, STRAND_NONE = 0, 1, 255


def strand_words(n_db: int) -> int:
    """uint64 words per row of the strand bitmap: bit d & 63 of word d >> 6 is the strand of database sequence d"""
    return (int(n_db) + 63) // 64


def _comp_table(comp) -> np.ndarray:
    table = np.ascontiguousarray(comp, dtype=np.uint8)
    if table.shape != (128,):
        raise AlignError(f"a complement table is 128 uint8, not {table.shape}")
    return table


def dna_complement() -> np.ndarray:
    """sa_dna_complement: the IUPAC complement table, 128 uint8 indexed by the residue's byte; 0: no complement"""
    comp = np.zeros(128, np.uint8)
    load_library().sa_dna_complement(comp.ctypes.data)
    return comp


def reverse_complement(store: SequenceStore, comp: Optional[np.ndarray] = None, scoring: Optional[Scoring] = None) -> SequenceStore:
    """sa_reverse_complement: a store of the same layout whose every sequence is reversed and mapped through `comp` (None:
    dna_complement()).  Raises AlignError naming the sequence and the byte for a residue without a complement, or -- with a
    scoring -- one whose complement the scoring's alphabet does not hold."""
    table = None if comp is None else _comp_table(comp)
    sc = None if scoring is None else scoring._as_c()
    blob = np.zeros_like(store.blob)
    if not load_library().sa_reverse_complement(store._as_c(), None if table is None else table.ctypes.data, None if sc is None else C.byref(sc),
                                                blob.ctypes.data):
        raise AlignError(_err())
    return SequenceStore(blob=blob, meta=store.meta.copy(), num=store.num, max=store.max)


def hip_search_strands(db: SequenceStore, queries: SequenceStore, scoring: Scoring, k: Optional[int] = None, rect: bool = False,
                       norm: Optional["Norm"] = None, pid: Optional[int] = None, comp: Optional[np.ndarray] = None):
    """sa_hip_search_strands: DNA queries against a database on both strands, folded on the first device.  With k: (index, value,
    score, strand) -- three (M, k) int32 arrays and one (M, k) uint8 (0 forward, 1 reverse); row q lists the database sequences by
    folded value descending, then index ascending.  With rect=True (rect, vrect, srect) follow: the folded (M, N) raw scores and
    values and the (M, N) uint8 strands.  The value is the raw score, or with norm=Norm(source, rule) the normalised score (the
    N + 2 M denominators are appended), or with pid=PID_* percent identity.  A cell is reverse iff its reverse value is larger."""
    n, m = db.num, queries.num
    if k is None and not rect:
        raise AlignError("hip_search_strands: nothing asked for (k is None and rect is False)")
    kk = 0 if k is None else _int32("k", k)
    index = value = score = strand = out = vout = sout = None
    if k is not None:
        rows = max(m, 1) * max(min(kk, NEIGHBORS_MAX), 1)
        index, value, score = (np.empty(rows, np.int32) for _ in range(3))
        strand = np.empty(rows, np.uint8)
    if rect:
        out, vout = (np.empty((max(m, 0), max(n, 0)), np.int32) for _ in range(2))
        sout = np.empty((max(m, 0), max(n, 0)), np.uint8)
    ptr = [None if a is None else a.ctypes.data for a in (index, value, score, strand, out, vout, sout)]
    table = None if comp is None else _comp_table(comp)
    sc = scoring._as_c()
    cn = den = None
    if norm is not None:
        cn, den = norm._as_c(n + 2 * m)
    cd = None if pid is None else C.c_int32(_denom(pid))
    if not load_library().sa_hip_search_strands(db._as_c(), queries._as_c(), C.byref(sc), None if table is None else table.ctypes.data, kk, *ptr,
                                                None if cn is None else C.byref(cn), None if cd is None else C.byref(cd)):
        raise AlignError(_err())
    res = ()
    if k is not None:
        res += tuple(a[:m * kk].reshape(m, kk) for a in (index, value, score, strand))
    if rect:
        res += (out, vout, sout)
    if den is not None:
        res += (den[:n + 2 * m],)
    return res


def last_search_strands_seconds() -> float:
    """device time of fold + strand take in the last hip_search_strands call, summed over its batches"""
    return float(load_library().sa_hip_last_search_strands_seconds())


def last_search_seconds() -> float:
    """device time of the last hip_search call: alignment + gather + selection, summed over its batches"""
    return float(load_library().sa_hip_last_search_seconds())


def last_search_quantity_seconds() -> float:
    """device time of denominators + sweep (norm=) or of the identity sweep (pid=) of the last hip_search call with a quantity,
    summed over its batches"""
    return float(load_library().sa_hip_last_search_quantity_seconds())


def last_search_breakdown() -> dict:
    a, g, h, b = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
    load_library().sa_hip_last_search_breakdown(C.byref(a), C.byref(g), C.byref(h), C.byref(b))
    return dict(align=float(a.value), gather=float(g.value), hits=float(h.value), batches=int(b.value))


class DeflateJob:
    """Device-side DEFLATE of a device-resident result matrix (sa_zjob_*, the -z option): the tiles (HDF5 chunks) of
    the full symmetric matrix as zlib streams (level 1..6: the fixed parse, 7..9: the pair parse, smaller) or as they are
    (level 0).  d_packed_ptr: scores by packed pair index; or d_full_ptr: N x N."""

    def __init__(self, num: int, chunk_dim: int, d_packed_ptr: int = 0, d_full_ptr: int = 0, device: int = 0, level: int = 6, _handle=None):
        self._lib = load_library()
        self._h = _handle or self._lib.sa_zjob_create(int(device), C.c_void_p(d_packed_ptr or None), C.c_void_p(d_full_ptr or None),
                                                      int(num), int(chunk_dim), int(level))
        if not self._h:
            raise AlignError(_err())
        self.tiles_per_row = int(self._lib.sa_zjob_tiles_per_row(self._h))
        self.num = int(num)

    @classmethod
    def begin(cls, store: "SequenceStore", scoring: "Scoring", chunk_dim: int, level: int = 6) -> "DeflateJob":
        """sa_hip_tiles_begin: the alignment of `store` runs on device 0 while next() hands out the finished tiles shell by shell"""
        lib = load_library()
        sc = scoring._as_c()
        h = lib.sa_hip_tiles_begin(store._as_c(), C.byref(sc), int(chunk_dim), int(level))
        if not h:
            raise AlignError(_err())
        job = cls(store.num, chunk_dim, _handle=h)
        job._store = store  # keep the host arrays alive
        return job

    def next(self) -> list[tuple[int, int, bytes]]:
        """the next batch of finished tiles as (tile row, tile column, bytes); [] when every tile has been handed out"""
        n = self.tiles_per_row
        rows, cols = (C.c_uint32 * n)(), (C.c_uint32 * n)()
        ptrs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
        got = self._lib.sa_zjob_next(self._h, rows, cols, ptrs, sizes)
        if got < 0:
            raise AlignError(_err())
        return [(int(rows[t]), int(cols[t]), C.string_at(ptrs[t], sizes[t])) for t in range(got)]

    @property
    def align_seconds(self) -> float:
        return float(self._lib.sa_zjob_align_seconds(self._h))

    def tile_row(self, row: int) -> list[bytes]:
        """the zlib streams of tile row `row` (copied out of the job's page-locked buffer)"""
        ptrs = (C.c_void_p * self.tiles_per_row)()
        sizes = (C.c_size_t * self.tiles_per_row)()
        if self._lib.sa_zjob_tile_row(self._h, int(row), ptrs, sizes):
            raise AlignError(_err())
        return [C.string_at(ptrs[t], sizes[t]) for t in range(self.tiles_per_row)]

    def neighbors(self, k: int) -> tuple[np.ndarray, np.ndarray]:
        """sa_zjob_neighbors: (index, score), two (N, k) int32 arrays, from the finished packed matrix this job's device
        holds -- after next() has returned [] for a begin() job; raises when the matrix is dealt over several jobs"""
        n, k = self.num, int(k)
        rows = max(n, 1) * max(min(k, NEIGHBORS_MAX), 1)
        index, score = np.empty(rows, np.int32), np.empty(rows, np.int32)
        if self._lib.sa_zjob_neighbors(self._h, k, index.ctypes.data, score.ctypes.data):
            raise AlignError(_err())
        return index[:n * k].reshape(n, k), score[:n * k].reshape(n, k)

    def edges(self, min_score: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """sa_zjob_edges: (offsets, index, score) as hip_edges returns them, from the finished packed matrix this job's device
        holds -- after next() has returned [] for a begin() job; raises when the matrix is dealt over several jobs"""
        return _take_edges(self._lib, self._lib.sa_zjob_edges(self._h, _min_score(min_score)))

    def linkage(self) -> tuple[np.ndarray, np.ndarray]:
        """sa_zjob_linkage: (pairs, score) as hip_linkage returns them, from the finished packed matrix this job's device
        holds -- after next() has returned [] for a begin() job; raises when the matrix is dealt over several jobs"""
        return _take_linkage(self._lib, self._lib.sa_zjob_linkage(self._h))

    def agglomerate(self, method) -> tuple[np.ndarray, np.ndarray]:
        """sa_zjob_agglomerate: (pairs, score) as hip_agglomerate returns them, from the finished packed matrix this job's
        device holds -- after next() has returned [] for a begin() job; raises when the matrix is dealt over several jobs"""
        return _take_linkage(self._lib, self._lib.sa_zjob_agglomerate(self._h, _agglo_method(method)))

    def select(self, ranks) -> tuple[np.ndarray, np.ndarray]:
        """sa_zjob_select: (values, below) as hip_select returns them, from the finished packed matrix this job's device
        holds -- after next() has returned [] for a begin() job; raises when the matrix is dealt over several jobs"""
        r = _ranks(ranks)
        value, below = _select_room(len(r))
        if self._lib.sa_zjob_select(self._h, r.ctypes.data, len(r), value.ctypes.data, below.ctypes.data):
            raise AlignError(_err())
        return value[:len(r)].copy(), below[:len(r)].copy()

    def normalize(self, norm: Norm) -> np.ndarray:
        """sa_zjob_normalize: normalises the finished matrix of a begin() job in place, once, after next() has returned [];
        neighbors / edges / linkage / select then answer over normalised scores (the tiles handed out stay raw).  Returns the
        denominators (N int32)."""
        cn, den = norm._as_c(self.num)
        if self._lib.sa_zjob_normalize(self._h, C.byref(cn)):
            raise AlignError(_err())
        return den[:self.num]

    def identity(self, denom: int) -> None:
        """sa_zjob_identity: overwrites the finished matrix of a begin() job with percent identity under `denom`, in place, once,
        after next() has returned []; neighbors / edges / linkage / select then answer over parts per million of identity (the
        tiles handed out stay raw)"""
        if self._lib.sa_zjob_identity(self._h, _denom(denom)):
            raise AlignError(_err())

    def stats(self) -> dict:
        e, c, r, o = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
        self._lib.sa_zjob_stats(self._h, C.byref(e), C.byref(c), C.byref(r), C.byref(o))
        return {"encode_ms": e.value, "copy_ms": c.value, "raw_bytes": r.value, "out_bytes": o.value}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.sa_zjob_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
