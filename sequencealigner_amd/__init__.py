"""sequencealigner_amd -- MI355X-native all-vs-all pairwise alignment (NW / Gotoh / SW score matrices).

Python mirror of the reference's device interface (jakovdev/SequenceAligner,
src/interface/seqalign_cuda.h) on top of the C ABI in include/seqalign_hip.h:

    reference (C)                                this package
    ------------------------------------------   ------------------------------------------
    struct input  {seqs, meta, max, num}         SequenceStore        (io/input.h:6-11)
    struct output {matrix, seqs, dim, triangular} numpy matrix + `triangular` flag (io/output.h:10-15)
    globals ALIGN/GAP_*/SEQ_LUT/SUB_MAT          Scoring              (bio/align.h:11-19)
    -a/-m/-p/-s/-e parse+validate                Scoring.from_names   (bio/align.c:87-142, bio/matrices.c:44-58)
    bool cuda_memory(size_t)                     hip_memory(bytes)    (seqalign_cuda.h:7)
    bool cuda_align(struct input, struct output) hip_align(store, scoring, triangular)  (seqalign_cuda.h:9)
    bool filter(struct input *)                  hip_filter(store, threshold)           (bio/filter.c:14)
    kernel(scores, start, batch)                 Context.align_range  (bio/align.h:48)

All compute happens in libseqalign_hip.so (hand-written HIP for gfx950).  There is no
Python/CPU fallback: a missing library or device raises.
"""
from .binding import (  # noqa: F401
    AlignError,
    Alignments,
    Context,
    DeflateJob,
    PinnedMatrix,
    Scoring,
    SequenceStore,
    device_count,
    device_name,
    last_align_breakdown,
    last_align_path,
    last_align_seconds,
    hip_align,
    hip_alignments,
    last_alignments_breakdown,
    last_alignments_seconds,
    hip_filter,
    hip_memory,
    hip_neighbors,
    last_neighbors_seconds,
    hip_edges,
    last_edges_seconds,
    hip_linkage,
    linkage_labels,
    linkage_merges,
    linkage_scratch_bytes,
    last_linkage_rounds,
    last_linkage_seconds,
    hip_select,
    hip_edges_at_rank,
    hip_linkage_with_ranks,
    score_rank,
    select_scratch_bytes,
    last_select_seconds,
    Norm,
    NORM_SELF,
    NORM_LENGTH,
    NORM_MIN,
    NORM_MAX,
    NORM_MEAN,
    NORM_SCALE,
    norm_value,
    last_normalize_seconds,
    PID_COLUMNS,
    PID_SHORTER,
    PID_LONGER,
    PID_MEAN,
    pid_value,
    hip_identity,
    last_identity_seconds,
    AGGLO_COMPLETE,
    AGGLO_AVERAGE,
    hip_agglomerate,
    hip_agglomerate_with_ranks,
    agglo_scratch_bytes,
    agglo_labels,
    last_agglomerate_seconds,
    last_agglomerate_rescans,
    SearchContext,
    hip_search,
    hits_scratch_bytes,
    last_search_seconds,
    last_search_breakdown,
    last_search_quantity_seconds,
    HitList,
    hip_search_above,
    hits_above_scratch_bytes,
    last_search_above_seconds,
    hip_search_strands,
    hip_search_above_strands,
    last_search_strands_seconds,
    hip_search_fit,
    last_search_fit_seconds,
    dna_complement,
    reverse_complement,
    strand_words,
    STRAND_FORWARD,
    STRAND_REVERSE,
    STRAND_NONE,
    library_path,
    load_library,
    matrix_names,
    method_names,
    pair_count,
    set_progress,
)

__all__ = [
    "AlignError", "Context", "PinnedMatrix", "Scoring", "SequenceStore", "device_count", "device_name", "last_align_breakdown", "last_align_path", "last_align_seconds", "hip_align", "hip_filter",
    "hip_memory", "hip_neighbors", "Alignments", "hip_alignments", "last_alignments_seconds", "last_alignments_breakdown", "last_neighbors_seconds", "hip_edges", "last_edges_seconds", "hip_linkage", "linkage_labels", "linkage_merges", "linkage_scratch_bytes", "last_linkage_rounds", "last_linkage_seconds", "hip_select", "hip_edges_at_rank", "hip_linkage_with_ranks", "score_rank", "select_scratch_bytes", "last_select_seconds", "Norm", "NORM_SELF", "NORM_LENGTH", "NORM_MIN", "NORM_MAX", "NORM_MEAN", "NORM_SCALE", "norm_value", "last_normalize_seconds", "PID_COLUMNS", "PID_SHORTER", "PID_LONGER", "PID_MEAN", "pid_value", "hip_identity", "last_identity_seconds", "AGGLO_COMPLETE", "AGGLO_AVERAGE", "hip_agglomerate", "hip_agglomerate_with_ranks", "agglo_scratch_bytes", "agglo_labels", "last_agglomerate_seconds", "last_agglomerate_rescans", "SearchContext", "hip_search", "hits_scratch_bytes", "last_search_seconds", "last_search_breakdown", "last_search_quantity_seconds", "HitList", "hip_search_above", "hits_above_scratch_bytes", "last_search_above_seconds", "hip_search_strands", "hip_search_above_strands", "last_search_strands_seconds", "hip_search_fit", "last_search_fit_seconds", "dna_complement", "reverse_complement", "strand_words", "STRAND_FORWARD", "STRAND_REVERSE", "STRAND_NONE", "library_path", "load_library", "matrix_names", "method_names", "pair_count", "set_progress",
]
