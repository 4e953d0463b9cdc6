/*
 * include/seqalign_hip.h -- C ABI of libseqalign_hip.so (MI355X / gfx950).
 *
 * Drop-in device boundary for the all-vs-all alignment hot path of
 * jakovdev/SequenceAligner.  Plain C: pointers, sizes and PODs only, no C++ or
 * torch types.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 * The reference keeps scoring state in process globals (GAP_PEN/GAP_OPN/GAP_EXT,
 * SEQ_LUT, SUB_MAT, ALIGN -- src/bio/align.h:11-19,28-42) and pushes it to the
 * device through the `pC` symbol (src/bio/kernels.cuh:12-25).  Here the same
 * state travels explicitly in `struct sa_scoring`; INTEGRATION.md shows the
 * five-line adapter that fills it from the reference's globals.
 *
 * Failure model: like the reference's CALLR/perr (src/interface/seqalign_cuda.c:23-30)
 * every call reports failure through its return value and leaves a human
 * readable message retrievable with sa_last_error() (also printed on stderr
 * when SA_HIP_VERBOSE is set).  There is NO CPU fallback anywhere behind this
 * ABI: no HIP device (or a missing code object) is an error, never a silent
 * host computation.
 */
#ifndef SEQALIGN_HIP_H
#define SEQALIGN_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_ABI_VERSION 4 /* 4: the sa_zjob_* / sa_hip_tiles_begin entry points; since then, additions only: the *_neighbors, *_alignments, *_edge*, *_linkage and *_select calls, then the *_norm* / *_denominators / *_normalize calls, then the *_identity* / *_pid* calls, then the *_agglo* calls, then the *_search* / *_hits calls, then the *_rect / _hits_take / sa_hip_search_norm / _pid calls, then the *_hits_above_* / sa_hip_search_above / sa_hitlist_* calls, then the *_strand* / sa_dna_complement / sa_reverse_complement calls */

/* ---- data types shared with the reference ------------------------------- */

/* src/bio/align.h:6-9  `struct meta` (byte offset into the blob, length w/o NUL) */
struct sa_meta {
	int32_t off;
	int32_t len;
};

/* src/io/input.h:6-11  `struct input`: one blob of uppercase residues, every
 * sequence NUL-terminated; meta[k] locates sequence k; max = longest len. */
struct sa_input {
	uint8_t *seqs;
	struct sa_meta *meta;
	int32_t max;
	int32_t num;
};

/* src/io/output.h:10-15  `struct output`.  matrix may be NULL (-W: compute,
 * copy nothing; src/interface/seqalign_cuda.c:233,268,279).
 * triangular: pair (i<j) at matrix[j*(j-1)/2 + i] (src/io/output.c:83);
 * otherwise full dim x dim, matrix[dim*i+j] = matrix[dim*j+i] = score and the
 * diagonal is left untouched (src/io/output.c:76-81). */
struct sa_output {
	int32_t *matrix;
	const char **seqs;
	size_t dim;
	bool triangular;
};

/* Alignment methods = entries of the reference's `aligns` registry
 * (src/bio/method/nw.c:46-51, ga.c:92-98, sw.c:66-71). */
enum sa_method { SA_METHOD_NW = 0, SA_METHOD_GA = 1, SA_METHOD_SW = 2, SA_METHOD_COUNT = 3 };
/* src/bio/align.h:34-37 */
enum sa_gap_kind { SA_GAP_LINEAR = 0, SA_GAP_AFFINE = 1 };

#define SA_LUT_SIZE 128 /* src/bio/align.h:11  SEQ_LUT_SIZE */
#define SA_SUB_DIM 24   /* src/bio/align.h:13  SUB_MAT_DIM  */
#define SA_SCORE_MIN (INT32_MIN / 2) /* src/bio/align.h:19 */

/* Replaces the globals read by cuda_align (src/interface/seqalign_cuda.c:115-123,170).
 * Gap values are the STORED form, i.e. already negated (src/bio/align.c:127-128):
 * `-p 4` -> gap_pen = -4; `-s 10 -e 1` -> gap_opn = -10, gap_ext = -1.
 *
 * `sub` is data: any 24 x 24 table may be given, symmetric or not (every named matrix is symmetric).  For the pair
 * (i, j), i < j, j the column sequence, the cell of residue x of i and residue y of j reads, as the reference does
 * (src/bio/method/nw.c:23,29; ga.c:46; sw.c:39):
 *     NW           sub[lut[x] * SA_SUB_DIM + lut[y]]      [code of i][code of j]
 *     Gotoh, SW    sub[lut[y] * SA_SUB_DIM + lut[x]]      [code of j][code of i]
 * Every kernel family and the traceback keep this order. */
struct sa_scoring {
	int32_t method;                        /* enum sa_method                   (ALIGN)    */
	int32_t gap_pen;                       /* linear gap, used by NW           (GAP_PEN)  */
	int32_t gap_opn;                       /* affine open, used by GA and SW   (GAP_OPN)  */
	int32_t gap_ext;                       /* affine extend, used by GA and SW (GAP_EXT)  */
	int32_t lut[SA_LUT_SIZE];              /* ASCII -> 0..23, -1 invalid       (SEQ_LUT)  */
	int32_t sub[SA_SUB_DIM * SA_SUB_DIM];  /* row-major 24x24                  (SUB_MAT)  */
};

/* ---- the two reference entry points ------------------------------------- */

/* Replaces `bool cuda_memory(size_t bytes)` (src/interface/seqalign_cuda.h:7,
 * src/interface/seqalign_cuda.c:71-93): true iff the device has bytes*4/3 free --
 * on EVERY device sa_hip_align will use (all visible ones, or the first SA_HIP_DEVICES).
 * Caller: output_load (src/io/output.c:37) to choose full vs triangular. */
bool sa_hip_memory(size_t bytes);

/* Replaces `bool cuda_align(struct input, struct output)`
 * (src/interface/seqalign_cuda.h:9, src/interface/seqalign_cuda.c:95-296).
 * Aligns every pair i<j of `in` and fills out.matrix in the layout out.triangular
 * selects.  Caller owns in/out for the duration of the call; all device memory
 * is allocated and released inside.  Uses every visible device when
 * SA_HIP_DEVICES is unset, or the first n with SA_HIP_DEVICES=n.  With several
 * devices the pair space is tiled over them (the job-wide tile list dealt by DP
 * work), the dense shares are all-gathered over RCCL so that every device holds
 * the whole matrix, and the host matrix is written once over all PCIe links;
 * when RCCL cannot be bound or the matrix does not fit a device, every device
 * delivers a contiguous slice instead (sa_hip_last_align_path tells which).
 * Never throws and never aborts the host process: any failure -- a C++
 * exception behind the boundary included -- is `false` + sa_last_error(). */
bool sa_hip_align(struct sa_input in, struct sa_output out, const struct sa_scoring *sc);

/* Device-assisted replacement of `bool filter(struct input *)` (src/bio/filter.c:14-89, the `-f` option):
 * keep[k] (in.num bytes) receives 1 for sequences that survive, 0 for dropped ones, with the reference's
 * SEQUENTIAL semantics (for j ascending, j is dropped iff some kept i<j has
 * matches(first min(len))/min(len) >= threshold in float).  The O(N^2 L) relation is computed on the device
 * as a bit matrix, the order-dependent keep/drop on the host.  Returns the number kept, <0 on error.
 * threshold <= 0 keeps everything (filter.c:16-17).  The caller compacts its store (filter.c:66-79). */
int32_t sa_hip_filter(struct sa_input in, float threshold, uint8_t *keep);

/* ---- device-resident layer (what sa_hip_align is built from) -------------
 * Used by multi-process drivers (one process per GPU + RCCL all-gather of the
 * packed slices, bench.py) and by callers that keep results in HBM. */

typedef struct sa_ctx sa_ctx;

/* Uploads the sequence store + scoring tables to `device` and plans the run
 * (src/interface/seqalign_cuda.c:115-132,168).  NULL on failure. */
sa_ctx *sa_ctx_create(int device, struct sa_input in, const struct sa_scoring *sc);
void sa_ctx_destroy(sa_ctx *ctx);

/* N(N-1)/2 (src/util/macros.h:13 `alignments`) */
int64_t sa_ctx_pairs(const sa_ctx *ctx);

/* Scores of packed pair indices [start, start+count) into DEVICE memory
 * d_scores[0..count) (= the reference's `kernel(scores, start, batch)`,
 * src/bio/align.h:48, src/bio/kernels.cu:32-40,73).  Asynchronous on `stream`
 * (a hipStream_t, NULL = default stream). 0 on success.
 * Calls of ONE context (this call, sa_ctx_align_range16, sa_ctx_align_share; all from one host thread at a time -- a context is
 * not thread-safe):
 *   in order on one stream   always fine, any number queued: every call takes its own tile counters from a ring, and a call that
 *                            reuses a slot waits, on its stream, for the slot's previous user.
 *   on several streams       fine when every range in flight runs on the packed and s32 TILE kernels alone -- no column sequence
 *                            longer than 1024 residues in it, and a scoring inside the systolic kernels' limits (sa_ctx_timing
 *                            names the kernels a range ran on: sa_k_systolic_pk_bundle<..> and sa_k_systolic<..,G..,K..> without
 *                            "strips").  Those launches touch nothing of the context but the call's own counters and read-only
 *                            tables.
 *                            NOT for a range with a strip-mined column (> 1024 residues) or a pair-per-wave run (a scoring beyond
 *                            those limits): these launches work in the context's one strip-boundary scratch, as
 *                            sa_ctx_identity_range, sa_ctx_denominators and sa_ctx_alignments do.  Such a call is ordered by
 *                            the caller -- one stream, or the caller's own events -- against every other call of the context
 *                            that uses the scratch.
 * The first call of a range builds and uploads its launch plan (blocking copies on the host; later calls of the range only
 * enqueue); a context keeps the plans of its 160 most recently used ranges, and building the 161st frees the oldest with
 * hipFree, which waits for the device. */
int sa_ctx_align_range(sa_ctx *ctx, int64_t start, int64_t count, int32_t *d_scores, void *stream);

/* Diagnostics: how the packed tiles of the context's LAST launch (range, share or host delivery batch) got their row tokens --
 * *lean from the token streams built beside the arranged copies of the store, *legacy derived from the code bytes in the
 * kernel (partial tiles, store-order tiles, everything with SA_HIP_NO_TOKENS=1).  Counted on the host from the launch plan
 * with the kernel's own rule.  0 on success. */
int sa_ctx_token_tiles(const sa_ctx *ctx, int64_t *lean, int64_t *legacy);

/* The launch/copy loop of cuda_align (src/interface/seqalign_cuda.c:182-292) on a ready context: scores of the
 * packed range [start, start+count) delivered into the HOST matrix `out` (the WHOLE matrix: packed element p
 * at out.matrix[p], or full dim x dim; out.matrix == NULL computes and copies nothing, the reference's -W).
 * Packed destination: double-buffered batches, each batch's device->host copy overlapping the next batch's
 * kernels.  Full destination with a column-aligned range and N^2 ints of free HBM: the L-shaped shell of every
 * column batch is expanded on the device and copied while the next batch computes; otherwise batches are
 * scattered by the host like output_fill (src/io/output.c:76-81).  Device buffers, streams and the page-locking
 * of a destination that is not yet page-locked are set up BEFORE the timed phase (the reference's allocations and
 * uploads are outside bench_align_start..end as well); *phase_seconds receives the duration of the loop itself.
 * sa_hip_align = sa_ctx_create + sa_ctx_align_host per device + sa_ctx_destroy.  0 on success. */
int sa_ctx_align_host(sa_ctx *ctx, int64_t start, int64_t count, struct sa_output out, double *phase_seconds);

/* Page-locks / releases a host range for device->host DMA (hipHostRegister).  A host that allocates its result
 * matrix once (output_load, src/io/output.c:55) registers it there; sa_ctx_align_host / sa_hip_align detect a
 * registered destination and skip their own temporary registration.  0 on success.  The range must be a mapping of
 * the caller's own -- start on a page boundary, outside the malloc heap, as output_load's mmap does: memory that malloc
 * manages is refused here and never page-locked by the library itself (a destination there is filled through the library's
 * pinned staging buffers); page-locking blocks that share pages with their heap neighbours is what both GPU memory faults
 * on this project's record have in common. */
int sa_hip_host_register(void *p, size_t bytes);
int sa_hip_host_unregister(void *p);

/* Exchange format for the multi-GPU all-gather (no reference counterpart: SURVEY 8e): the same scores as
 * int16 when they provably fit -- every |score| <= max_len * max|S| + 2 * max_len * max|gap| <= 32767 for this
 * store and scoring (sa_ctx_scores_fit16) -- so that the collective moves half the bytes; sa_hip_widen16 turns
 * the gathered vector back into the reference's s32 on the device.  sa_ctx_align_range16 fails when the bound
 * does not hold. */
int sa_ctx_scores_fit16(const sa_ctx *ctx);
int sa_ctx_align_range16(sa_ctx *ctx, int64_t start, int64_t count, int16_t *d_scores, void *stream);
int sa_hip_widen16(const int16_t *d_src, int32_t *d_dst, int64_t count, void *stream);

/* Tile-interleaved sharding for one process per GPU (no reference counterpart: SURVEY 8e; replaces the contiguous
 * range abstraction `kernel(scores, start, batch)` of src/bio/kernels.cu:32-40 in the multi-GPU path).  The launch
 * plan of the packed range [start, start+count) -- the largest-first list of workgroup-tiles of every column-length
 * class -- is the same on every rank; its tiles are dealt over `world` ranks by accumulated DP work, so every rank
 * keeps full-size tiles and whole arranged row blocks.  Rank `rank` scores its tiles and stores them densely, in tile
 * order, into d_share: sa_ctx_share_elems() elements (the same on every rank) of int16 (elem16 != 0; needs
 * sa_ctx_scores_fit16) or s32.  After an all-gather of the shares (rank-major, world x share_elems elements),
 * sa_ctx_place_shares widens and places them: d_packed[p - start] = score of pair p, the reference's packed order
 * (src/io/output.c:83).  Host delivery (the device->host copies inside the reference's timed loop,
 * src/interface/seqalign_cuda.c:266-283): with host_packed != NULL -- the WHOLE packed host matrix, page-locked
 * (sa_hip_host_register), e.g. one shared mapping all ranks of a node attach -- the kernels of a rank also store its
 * own scores straight into host_packed[p], as sa_ctx_align_host does for one device: together the ranks fill the
 * matrix exactly once, with no copy pass and without waiting for the gather.  `to_host` of the other two calls must
 * say whether the shares are computed that way (the plan differs: tiles are then their own arranged row blocks).
 * world = 1 is allowed (one share holding every tile).  All asynchronous on `stream`. */
int64_t sa_ctx_share_elems(sa_ctx *ctx, int64_t start, int64_t count, int world, int to_host);
int sa_ctx_align_share(sa_ctx *ctx, int64_t start, int64_t count, int world, int rank, void *d_share, int elem16,
		       int32_t *host_packed, void *stream);
int sa_ctx_place_shares(sa_ctx *ctx, int64_t start, int64_t count, int world, int to_host, const void *d_shares, int elem16,
			int32_t *d_packed, void *stream);

/* on != 0: the launches this context issues from now on run three instead of four persistent workgroups per CU, leaving
 * LDS and wave slots for kernels of OTHER streams to run beside them -- the RCCL all-gather and sa_ctx_place_shares of the
 * previous super-chunk in an overlapped multi-GPU schedule.  (Four per CU fill the LDS: a concurrent kernel then waits
 * for the launch to end.)  Costs the NW kernels ~8 %, Gotoh / SW ~1 %; off by default. */
void sa_ctx_leave_room(sa_ctx *ctx, int on);

/* Packed triangular (device) -> full symmetric dim x dim with zero diagonal
 * (device), the layout of src/io/output.c:76-81.  Asynchronous on `stream`. */
int sa_ctx_expand_full(sa_ctx *ctx, const int32_t *d_packed, int32_t *d_full, void *stream);

/* ---- compressed output on the device (the -z option) ----------------------
 * The reference asks libhdf5 for DEFLATE on the chunked /similarity_matrix (src/io/format/hdf5.c:91-95) and H5Dwrite
 * (:148-194) then deflates every chunk in the one writing thread -- for BASELINE config 5 (89 994 sequences, 484 chunks
 * of 4096 x 4096, level 6) 41 CPU-minutes behind a two-second alignment.  Here the chunks ("tiles") are encoded where
 * the scores are: a job walks the tile rows of the full symmetric matrix (zero diagonal, zeros beyond N: exactly what
 * H5Dwrite hands the filter) over a DEVICE-resident matrix -- packed by pair index (d_packed) or full N x N (d_full,
 * used when d_packed is NULL) -- and returns every tile as a complete zlib stream (RFC 1950 / 1951) in page-locked host
 * memory, ready for H5Dwrite_chunk (filter mask 0); any inflate reads them.  `level` chooses the parse:
 * 1 .. 6 the fixed parse (every element by itself: its low byte, then a length-3 match onto one of its eight predecessors;
 * the ratio on score matrices sits between zlib -1 and -4), SA_HIP_Z_PAIR_LEVEL .. 9 the pair parse (8-byte matches onto
 * equal pairs of elements anywhere in the 32 KB of the tile before them, found by one more kernel; 5 to 7 % fewer bytes
 * on NW scores, between zlib -4 and -6, at about twice the encoder time, for two more bytes of device memory per element of a line of tiles).  The same
 * level on the same matrix gives the same bytes, run after run.  Level 0 returns the
 * tiles as they are (chunk_dim^2 int32 each), for a chunked dataset without filters: the same H5Dwrite_chunk loop then
 * replaces H5Dwrite's gather of every tile out of N-wide rows in the writing thread (hdf5.c:148-194).
 *   sa_zjob_create       buffers for one line of tiles; chunk_dim: a power of two in [64, 4096] (sa_host_hdf5_chunk_dim)
 *   sa_zjob_tile_row     streams[t] / sizes[t] for the tiles_per_row tiles of row `tile_row`, valid until the next call;
 *                        rows are asked for in order, each once: the next row is encoded while the caller writes
 *   sa_hip_tiles_begin   sa_ctx_create + the packed matrix in device memory + a job that walks the tiles in
 *                        SHELLS while the alignment is still running: the tiles whose larger tile index is b need exactly
 *                        the columns [b * chunk_dim, (b + 1) * chunk_dim), so they are encoded and handed out while the
 *                        device aligns the next column blocks (the alignment phase and the reference's output phase,
 *                        src/main.c:31-34, overlap).  The first blocks are on their way when it returns.  With several
 *                        devices (all visible ones, or the first SA_HIP_DEVICES) block b and its shell belong to device
 *                        b mod n: a shell needs nothing but its own block, so the devices exchange nothing and every one
 *                        drives its own PCIe link; the shells still come in ascending order.
 *   sa_zjob_next         the next batch of finished tiles (at most tiles_per_row): rows[t], cols[t] = tile coordinates,
 *                        streams[t] / sizes[t] valid until the next call; returns their number, 0 when every tile has been
 *                        handed out, < 0 on error.  Works on a sa_zjob_create job as well (then: row after row).
 *   sa_zjob_align_seconds  device time of the alignment so far (sum over the finished column blocks: the bracket of
 *                        sa_hip_last_align_seconds).
 * NULL / non-zero + sa_last_error on failure. */
#define SA_HIP_Z_PAIR_LEVEL 7 /* levels from here on: the pair parse */
typedef struct sa_zjob sa_zjob;
sa_zjob *sa_zjob_create(int device, const int32_t *d_packed, const int32_t *d_full, int32_t num, size_t chunk_dim, int level);
size_t sa_zjob_tiles_per_row(const sa_zjob *job);
int sa_zjob_tile_row(sa_zjob *job, size_t tile_row, const uint8_t **streams, size_t *sizes);
int sa_zjob_next(sa_zjob *job, uint32_t *rows, uint32_t *cols, const uint8_t **streams, size_t *sizes);
void sa_zjob_stats(const sa_zjob *job, double *encode_ms, double *copy_ms, uint64_t *raw_bytes, uint64_t *out_bytes);
double sa_zjob_align_seconds(const sa_zjob *job);
void sa_zjob_destroy(sa_zjob *job);
sa_zjob *sa_hip_tiles_begin(struct sa_input in, const struct sa_scoring *sc, size_t chunk_dim, int level);

/* ---- nearest neighbours: the k best partners of every sequence, selected on the device ---------------------------
 * No reference counterpart: the reference delivers the N x N matrix, and whoever clusters, builds a graph or looks up
 * nearest hits sorts every row of it on the host.  The scores sit in device memory when the alignment ends; selecting
 * there reads them once and returns N x k indices and N x k scores.
 * Contract: the candidates of sequence r are all c != r with score(r, c), the symmetric matrix entry (the diagonal is not a
 * candidate); larger is better for all three methods.  Order: score DESCENDING, then index c ASCENDING.  Row r of the
 * result holds the first k candidates in that order: index[r * k + t], score[r * k + t], t = 0 .. k - 1.  The tie rule is
 * part of the contract: the same store and scoring give the same bytes run after run.
 * 1 <= k <= min(N - 1, SA_HIP_NEIGHBORS_MAX); anything else is an error through sa_last_error(). */
#define SA_HIP_NEIGHBORS_MAX 64
/* device-resident: d_packed = whole packed matrix of ctx's store; d_index, d_score: N*k int32 each, device memory.
 * Asynchronous on `stream`.  Needs no scratch memory. */
int sa_ctx_neighbors(sa_ctx *ctx, const int32_t *d_packed, int32_t k, int32_t *d_index, int32_t *d_score, void *stream);
/* one call, host in / host out: align into device memory, select, copy back 2*N*k ints.  The matrix never leaves the
 * device and no host matrix exists.  One device (the first).  Fails cleanly when the packed matrix does not fit.
 * sa_hip_last_align_seconds() then tells the device time of the alignment inside it. */
bool sa_hip_neighbors(struct sa_input in, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score);
/* on a tile job whose device holds the finished packed matrix.  For sa_hip_tiles_begin on one device: after
 * sa_zjob_next has returned 0.  For sa_zjob_create with d_packed: any time.  Host arrays out.  Non-zero + sa_last_error
 * when the job does not hold the whole matrix on one device (several devices, SA_HIP_TILES_SPLIT > 1, a d_full job). */
int sa_zjob_neighbors(sa_zjob *job, int32_t k, int32_t *index, int32_t *score);
/* device time (seconds) of the selection kernel in the last successful sa_hip_neighbors / sa_zjob_neighbors call */
double sa_hip_last_neighbors_seconds(void);

/* ---- search: queries against a database, the k best hits of every query selected on the device -----------------------
 * No reference counterpart: the reference scores one store against itself.  Let db (N >= 1 sequences) and queries (M >= 1)
 * be two stores; the CONCATENATED store is db followed by queries.  The score of query q against database sequence d is the
 * similarity-matrix entry of pair (d, N + q) of the concatenated store: d is the row sequence, the query the column
 * sequence, and the substitution table is indexed exactly as struct sa_scoring documents -- with an asymmetric table the
 * search of A against B is not the search of B against A.  Only the M * N query-database pairs are computed; no pair of two
 * queries and no pair of two database sequences is.
 *   rect   int32 M x N, row-major: rect[q * N + d]
 *   hits   the candidates of query q are ALL d in [0, N) (the stores are separate: there is no self to exclude); order: score
 *          DESCENDING, then d ASCENDING; row q of index / score (M x k) holds the first k.  1 <= k <= min(N,
 *          SA_HIP_NEIGHBORS_MAX).  The tie rule is part of the contract: the same inputs give the same bytes run after run.
 *   alignments of hits   sa_ctx_alignments on the search context with a = N + q, b = d.  a > b, so the record comes back
 *          mirrored as that call documents: the a_* spans are the query's, SA_ALN_I is a residue of the query only, and
 *          `score` equals rect[q * N + d].
 *
 * sa_ctx_create_search concatenates the two stores on the host and is otherwise sa_ctx_create; the context's launch plans are
 * bounded to the database rows.  NULL + sa_last_error for an empty store, or when N + M or the concatenated blob passes the
 * int32 of struct sa_meta.  sa_ctx_search_db / _queries: N and M, or 0 for a context of sa_ctx_create.
 * A search context has no packed triangle: every sa_ctx_* call over a packed range or a packed matrix (sa_ctx_align_range /
 * _range16 / _host / _share, _share_elems, _place_shares, _expand_full, _identity_range, _neighbors, _edge_*, _linkage,
 * _agglomerate, _select, _normalize) refuses it with one message that names sa_ctx_search_range.  sa_ctx_alignments,
 * sa_ctx_timing, sa_ctx_timing_read and sa_ctx_token_tiles work.  The calls that take no context but a packed matrix and its
 * order (sa_zjob_create and what follows from it) know nothing of contexts: there is no packed matrix of a search to hand them,
 * and a rectangle passed as one is the caller's error, undefined as any wrong pointer is.
 *
 * sa_ctx_search_range   queries [q0, q0 + nq) into dense DEVICE memory d_rect[(q - q0) * N + d].  Asynchronous on `stream`,
 *          allocates nothing.  d_scratch: sa_search_scratch_bytes(ctx, q0, nq) bytes of device memory -- the bounded packed
 *          range [tri(N + q0), tri(N + q0 + nq)) lands there, row q at pitch N + q, and a gather kernel moves the rows to
 *          pitch N (the score kernels place scores by packed index; dense stores straight from them are not built).
 * sa_ctx_hits   the hits of rows [0, nq) of a device rectangle of pitch N = sa_ctx_search_db(ctx): d_index, d_score nq * k
 *          int32 each, device memory.  Asynchronous on `stream`, allocates nothing, leaves d_rect unchanged.  d_scratch:
 *          sa_hits_scratch_bytes(N, nq, k) bytes of device memory, 8-byte aligned (refused otherwise); that is 0, and d_scratch may be NULL, when the rows alone
 *          fill the device (with few rows every row is cut into segments whose partial lists go through the scratch).
 * sa_hip_search   one call, host in / host out, one device (the first).  rect may be NULL; index and score may both be NULL
 *          when rect is not (k is then ignored).  The queries go in batches sized from the free device memory
 *          (SA_HIP_SEARCH_BATCH_BYTES=n caps the device buffers that grow with a batch), so any M works.  Arguments are checked
 *          before a device is looked for.
 * sa_hip_last_search_seconds / _breakdown   device time of the last successful sa_hip_search, summed over its batches:
 *          alignment, gather, selection; and the number of batches.
 * Non-zero / false / NULL + sa_last_error on failure. */
sa_ctx *sa_ctx_create_search(int device, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc);
int32_t sa_ctx_search_db(const sa_ctx *ctx);
int32_t sa_ctx_search_queries(const sa_ctx *ctx);
size_t sa_search_scratch_bytes(const sa_ctx *ctx, int32_t q0, int32_t nq);
int sa_ctx_search_range(sa_ctx *ctx, int32_t q0, int32_t nq, int32_t *d_rect, void *d_scratch, void *stream);
size_t sa_hits_scratch_bytes(int32_t n_db, int32_t nq, int32_t k);
int sa_ctx_hits(sa_ctx *ctx, const int32_t *d_rect, int32_t nq, int32_t k, int32_t *d_index, int32_t *d_score, void *d_scratch, void *stream);
bool sa_hip_search(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score,
		   int32_t *rect);
double sa_hip_last_search_seconds(void);
void sa_hip_last_search_breakdown(double *align, double *gather, double *hits, int32_t *batches);

/* ---- search: hits ranked by a value -- normalised score or percent identity -- instead of the raw score ---------------------
 * No reference counterpart.  A raw score grows with length: against a database of mixed lengths the k "best" hits of a query are
 * led by the long entries, and "which database sequences are at least 90 % identical to my query" cannot be asked.  The
 * quantities are the ones the all-vs-all selections read ("normalised scores" and "percent identity" below), at rectangle pitch.
 * Pair and orientation: for query q and database sequence d the pair is (d, N + q) of the concatenated store, already canonical:
 * i = d is the row sequence, j = N + q the column sequence.  Values are in parts per million (SA_NORM_SCALE):
 *   normalised   sa_norm_value(rect[q * N + d], den[d], den[N + q], rule); den holds the N + M denominators of the concatenated
 *                store.  sa_ctx_denominators on a search context gives exactly these N + M (d_den: N + M int32); a caller may
 *                pass denominators of their own.
 *   identity     sa_pid_value(identities, columns, len_d, len_query, denom) of the canonical alignment of (d, N + q): exactly the
 *                numbers sa_ctx_identity_range gives that pair on a context of the concatenated store.
 * Hits by value: all d in [0, N) ordered value DESCENDING, then d ASCENDING, the first k taken -- the key of sa_ctx_hits,
 * unchanged: sa_ctx_hits over a value rectangle selects them.  Every hit also carries its raw score (sa_ctx_hits_take).
 *
 * sa_ctx_normalize_rect   device-resident, asynchronous on `stream`, no scratch, no host synchronisation: rows [0, nq) of a
 *          rectangle of pitch N whose row r is query q0 + r: d_out[r * N + d] = value of d_rect[r * N + d].  d_den: N + M int32 of
 *          device memory.  d_out == d_rect (in place) or disjoint; partial overlap is the caller's error.  4-byte alignment is
 *          enough (an offset view will do).  Refused before any launch: a context of sa_ctx_create, a null pointer, a rule outside
 *          its enum, q0 < 0, nq < 1 or q0 + nq > M, a misaligned pointer.
 * sa_ctx_identity_rect   the dense form of sa_ctx_identity_range for a search context: queries [q0, q0 + nq), element
 *          (q - q0) * N + d of every non-NULL output of *d_out.  Same struct, same subset rule, same refusals (and a context of
 *          sa_ctx_create, queries outside [0, M)); like that call it uses the context's strip-boundary scratch and payload buffer
 *          and does not run beside sa_ctx_search_range, sa_ctx_denominators or another identity call of the SAME context on
 *          another stream; in order on one stream is fine.
 * sa_ctx_hits_take   d_out[r * k + t] = d_rect[r * N + d_index[r * k + t]] for rows [0, nq): the raw scores of hits that were
 *          selected on a value rectangle.  An index outside [0, N) reads nothing and gives INT32_MIN.  nq and k as sa_ctx_hits.
 * sa_hip_search_norm / _pid   one call, host in / host out, first device.  index, value, score are M x k; rect holds the raw
 *          scores and vrect the values, both M x N.  Any of value, score, rect, vrect may be NULL; index may be NULL only when
 *          nothing M x k is wanted.  Row q of index / value is ordered by value descending, then index ascending; score is the raw
 *          score of each hit and is not sorted.  norm == NULL is exactly sa_hip_search, with value a copy of score and vrect a
 *          copy of rect.  norm->denominators, when not NULL, receives N + M values.  _pid runs no packed alignment: the identity
 *          sweep delivers score and pid together.  Stream order, norm: range, rows to pitch N, denominators (once per call),
 *          sweep into the value rectangle, sa_ctx_hits on it, take; pid: identity sweep, hits, take.  The queries go in batches
 *          sized as sa_hip_search sizes them with the extra rectangle counted -- per query 4 (N + M) bytes (norm only) + 8 N +
 *          20 k (with hits) -- and SA_HIP_SEARCH_BATCH_BYTES caps a batch.  Every argument is checked before a device is looked
 *          for.
 * sa_hip_last_search_quantity_seconds   the device time of denominators + sweep, or of the identity sweep, summed over the
 *          batches of the last successful sa_hip_search_norm / _pid call (0 after norm == NULL).  sa_hip_last_search_seconds /
 *          _breakdown answer for these calls as well: alignment (under percent identity the sweep itself, which delivers the
 *          scores), gather, selection + take, batches; the quantity's time is not in them except in that case.
 * Non-zero / false + sa_last_error on failure. */
struct sa_norm;
struct sa_identity_out;
int sa_ctx_normalize_rect(sa_ctx *ctx, const int32_t *d_rect, int32_t nq, int32_t q0, const int32_t *d_den, int32_t rule, int32_t *d_out,
			  void *stream);
int sa_ctx_identity_rect(sa_ctx *ctx, int32_t q0, int32_t nq, const struct sa_identity_out *d_out, void *stream);
int sa_ctx_hits_take(sa_ctx *ctx, const int32_t *d_rect, int32_t nq, int32_t k, const int32_t *d_index, int32_t *d_out, void *stream);
bool sa_hip_search_norm(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *value,
			int32_t *score, int32_t *rect, int32_t *vrect, const struct sa_norm *norm);
bool sa_hip_search_pid(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *value,
		       int32_t *score, int32_t *rect, int32_t *vrect, int32_t denom);
double sa_hip_last_search_quantity_seconds(void);

/* ---- search: every hit at or above a threshold, as a CSR over the rows of the rectangle -----------------------------------------
 * No reference counterpart.  The k best hits answer "who is closest"; "which database sequences are at least 90 % identical to
 * my query" has no fixed length per query and no bound of 64.  Let vrect be a device rectangle of pitch N whose values are raw
 * scores, normalised scores or percent identity in parts per million, and min_value any int32.  Database sequence d is a hit of
 * row r iff vrect[r * N + d] >= min_value.  The result is a CSR over the rows:
 *   offsets  int64[nq + 1], offsets[0] = 0, offsets[r + 1] - offsets[r] = hits of row r, offsets[nq] = E
 *   index    int32[E], row r's hits in ASCENDING d (ranking best-first is what the k best hits are for)
 *   value    int32[E], vrect at each hit
 *   score    int32[E], the raw-score rectangle rect at each hit
 * INT32_MIN gives E = nq * N; a threshold above the maximum gives a valid empty result (all offsets 0).  No position depends on
 * which wave arrives first: the same inputs give the same bytes.  Offsets, and everything computed from them, are 64-bit.
 *
 * Both device-resident calls are asynchronous on `stream`, allocate nothing and do not synchronise with the host; both leave
 * their input rectangles unchanged.  Refused before any launch: a context of sa_ctx_create, a null required pointer, nq outside
 * [1, M], a scratch that is not 8-byte aligned.
 * sa_hits_above_scratch_bytes   host only: bytes of d_scratch for rows [0, nq) of a rectangle of pitch n_db -- 8 * (nq * S + 1),
 *          S the segments a row is cut into, a function of (n_db, nq) alone.  0 for n_db < 1 or nq < 1.
 * sa_ctx_hits_above_offsets   count + scan: d_offsets (nq + 1 int64 of device memory) for rows [0, nq) of d_vrect.  d_scratch
 *          receives the place of every segment's first hit and belongs to the fill that follows.
 * sa_ctx_hits_above_fill   d_index (required), d_value, d_score (each may be NULL): E int32 each, E = d_offsets[nq], which the
 *          caller has read to size them.  d_offsets and d_scratch as _offsets left them for the SAME d_vrect, nq and min_value.
 *          d_rect is read iff d_score is not NULL, at the hits only, and may equal d_vrect.  A row never writes at or beyond
 *          d_offsets[r + 1], whatever the caller handed in.
 * sa_hip_search_above   one call, host in / host out, first device.  norm and pid_denom both NULL: raw scores, value == score;
 *          norm: normalised scores (norm->denominators, when not NULL, receives N + M values); pid_denom: percent identity under
 *          *pid_denom; both given: refused.  Every argument is checked before a device is looked for.  The queries go in batches
 *          sized as sa_hip_search_norm / _pid size them, with the scratch of this call in place of the hit lists -- per query
 *          4 (N + M) bytes (not under percent identity) + 4 N (raw scores) or 8 N + 8 -- and SA_HIP_SEARCH_BATCH_BYTES caps a
 *          batch.  Stream order per batch: range, rows to pitch N, the quantity's sweep (or the identity sweep alone), count +
 *          scan, the host reads E of the batch, an exact device buffer for its hits (the largest so far is kept), fill, copy into
 *          host arrays that grow.  A batch whose hits do not fit the device or the host gives NULL + sa_last_error naming the
 *          queries, E and the bytes; the process goes on working.  The result owns its arrays until sa_hitlist_destroy.
 * sa_hip_last_search_above_seconds   device time of count + scan + fill, summed over the batches of the last successful
 *          sa_hip_search_above.  sa_hip_last_search_seconds / _breakdown / _quantity_seconds answer as after sa_hip_search_norm /
 *          _pid; the `hits` part of the breakdown is this call's count + scan + fill.
 * Non-zero / NULL + sa_last_error on failure. */
size_t sa_hits_above_scratch_bytes(int32_t n_db, int32_t nq);
int sa_ctx_hits_above_offsets(sa_ctx *ctx, const int32_t *d_vrect, int32_t nq, int32_t min_value, int64_t *d_offsets, void *d_scratch,
			      void *stream);
int sa_ctx_hits_above_fill(sa_ctx *ctx, const int32_t *d_vrect, const int32_t *d_rect, int32_t nq, int32_t min_value, const int64_t *d_offsets,
			   const void *d_scratch, int32_t *d_index, int32_t *d_value, int32_t *d_score, void *stream);
typedef struct sa_hitlist sa_hitlist; /* owns offsets / index / value / score in host memory, like sa_edges */
sa_hitlist *sa_hip_search_above(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t min_value,
				const struct sa_norm *norm, const int32_t *pid_denom);
const int64_t *sa_hitlist_offsets(const sa_hitlist *h, int32_t *queries); /* M + 1 entries; *queries (may be NULL) = M */
const int32_t *sa_hitlist_index(const sa_hitlist *h, int64_t *count);     /* *count (may be NULL) = E; never NULL for a valid result */
const int32_t *sa_hitlist_value(const sa_hitlist *h);
const int32_t *sa_hitlist_score(const sa_hitlist *h);
void sa_hitlist_destroy(sa_hitlist *h);
double sa_hip_last_search_above_seconds(void);

/* ---- search: both strands of DNA queries, folded on the device ------------------------------------------------------------------
 * No reference counterpart.  A read comes from either strand of its source; a search that aligns every query as written finds no
 * homologue for about half of a sequencing run.  A STRANDS context holds db (N), the M queries and the M reverse complements of
 * the queries as one search context: sa_ctx_search_queries answers 2 M, row M + q of any rectangle is query q reversed and
 * complemented, and every search call above (sa_ctx_search_range, _normalize_rect, _identity_rect, sa_ctx_denominators -- N + 2 M
 * values --, sa_ctx_hits, _hits_take, _hits_above_*, sa_ctx_alignments) works on those rows unchanged: they are simply more rows.
 * No alignment kernel knows of strands.
 *
 * Complement: sa_dna_complement fills the IUPAC table over the upper-case nucleotide alphabet of the shipped tables,
 * ATGCSWRYKMBVHDN*: A<->T, G<->C, R<->Y, K<->M, B<->V, H<->D; S, W, N and * map to themselves; U -> A; every other byte maps to
 * 0, "no complement".  sa_reverse_complement writes, for every sequence of `in`, its residues reversed and mapped through comp
 * (NULL: sa_dna_complement's) into blob_out at the SAME offsets, the NUL terminators included: the same meta serves, blob_out
 * spans what in.seqs spans and may not be in.seqs.  false + sa_last_error naming the sequence (#1 is the first), the residue and the
 * byte for a residue whose complement is 0, and for one whose complement sc->lut rejects (sc may be NULL: not checked).
 *
 * Fold: v_fwd = value of row q, v_rev = value of row M + q, for the same d.  The cell is REVERSE iff v_rev > v_fwd; equal values
 * keep the forward strand, whatever the raw scores are.  The folded value is the larger value, the folded raw score the raw score
 * of the strand that won.  Strand bitmap: (N + 63) / 64 uint64 words per row; bit d & 63 of word d >> 6 of row r is the strand of
 * cell (r, d), SA_STRAND_FORWARD = 0, SA_STRAND_REVERSE = 1; bits at or beyond N are zero.
 *
 * sa_ctx_create_search_strands   builds the reverse complements on the host (comp == NULL: sa_dna_complement) and is otherwise
 *          sa_ctx_create_search.  NULL + sa_last_error, before a device is looked for: a residue that cannot be complemented, as
 *          above; N + 2 M or the concatenated blob past the int32 of struct sa_meta.
 * sa_ctx_search_strands   2 for such a context, 1 for a context of sa_ctx_create_search, 0 otherwise.
 * The three device-resident calls are asynchronous on `stream`, allocate nothing, never synchronise with the host, use no
 * atomics and give the same bytes run after run.  Each refuses, before any launch: a context that is not a strands context, a
 * null required pointer, nq outside [1, M], a bitmap pointer that is not 8-byte aligned, a rectangle or index that is not 4-byte
 * aligned (offsets: 8-byte).  Rectangles need no more than 4-byte alignment (an offset view will do).
 * sa_ctx_strand_fold   rows [0, nq) at pitch N: d_vfwd / d_vrev are the value rectangles of the two strands and decide; d_sfwd /
 *          d_srev / d_sbest, the raw-score rectangles, are carried along -- all three given or all three NULL (the raw-score
 *          search, where value is score).  d_vbest may be d_vfwd and d_sbest may be d_sfwd (in place); any other overlap is the
 *          caller's error.  d_bits (nq * ((N + 63) / 64) uint64) may be NULL.  One streaming kernel.
 * sa_ctx_hits_strand   d_strand[r * k + t] (uint8) = the bit of cell (r, d_index[r * k + t]) for rows [0, nq) of an M x k hit list;
 *          an index outside [0, N) reads nothing and gives SA_STRAND_NONE = 255.  nq and k as sa_ctx_hits.
 * sa_ctx_hits_above_strand   the same for a CSR: row r owns entries d_offsets[r] .. d_offsets[r + 1] of d_index / d_strand;
 *          offsets are 64-bit throughout, and E is read on the device only.
 * sa_hip_search_strands   one call, host in / host out, first device.  index, value, score are M x k int32, strand M x k uint8;
 *          rect and vrect are the FOLDED M x N rectangles of raw scores and values, srect the M x N strands, one uint8 per cell.
 *          Any output may be NULL; index may be NULL only when nothing M x k is wanted.  norm and pid_denom both NULL: raw scores,
 *          value == score; norm: normalised scores (norm->denominators, when not NULL, receives N + 2 M values: database, queries,
 *          reverse complements); pid_denom: percent identity under *pid_denom; both: refused.  Order inside a row: value descending,
 *          then index ascending -- the key of sa_ctx_hits.  Stream order per batch of queries [q0, q0 + nq): the forward rows, the
 *          rows M + q0 .., each through the calls of sa_hip_search / _norm / _pid; fold in place; sa_ctx_hits on the folded values;
 *          the raw scores and the strands of the hits.  Batches are sized as sa_hip_search sizes them, with both strands counted --
 *          per query 4 (N + 2 M) bytes (the range row, which the two halves use in turn; not under percent identity) + 8 N (raw
 *          scores) or 16 N (a quantity: two rectangles per strand) + 8 ((N + 63) / 64) (the bitmap) + 21 k (with hits) -- and
 *          SA_HIP_SEARCH_BATCH_BYTES caps a batch.  Every argument is checked before a device is looked for.
 * sa_hip_search_above_strands   the threshold form over the folded values: sa_hip_search_above with both strands.  Stream order per
 *          batch: both halves of the rows, the quantity's sweeps, fold in place, count + scan, the host reads E, fill, the strands of
 *          the entries.  Per query 4 (N + 2 M) bytes (not under percent identity) + 8 N (raw scores) or 16 N (a quantity) + 8 ((N + 63) / 64) (the
 *          bitmap) + 8 (scratch).
 *          sa_hitlist_strand: uint8[E], the strand of every hit; NULL for a list of sa_hip_search_above.  value and score are those
 *          of the strand that won.
 * sa_hip_last_search_strands_seconds   device time of fold + strand take, summed over the batches of the last successful
 *          sa_hip_search_strands / sa_hip_search_above_strands.  sa_hip_last_search_seconds / _breakdown / _quantity_seconds answer for the rest as after
 *          sa_hip_search_norm / _pid, with both halves of the alignment (and of the gather, and of the quantity) summed.
 * Alignments of hits need no new call: on a strands context sa_ctx_alignments with a = N + q, b = d aligns a forward hit and
 *          a = N + M + q, b = d a reverse hit; `score` equals the folded rect[q * N + d] when the strand is the hit's own.  For a
 *          reverse hit the a_* spans and the CIGAR refer to the REVERSE COMPLEMENT of the query: position p there is position
 *          len - 1 - p of the query as given.
 * Non-zero / false / NULL + sa_last_error on failure. */
#define SA_STRAND_FORWARD 0
#define SA_STRAND_REVERSE 1
#define SA_STRAND_NONE 255
void sa_dna_complement(uint8_t comp[SA_LUT_SIZE]);
bool sa_reverse_complement(struct sa_input in, const uint8_t *comp, const struct sa_scoring *sc, uint8_t *blob_out);
sa_ctx *sa_ctx_create_search_strands(int device, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp);
int32_t sa_ctx_search_strands(const sa_ctx *ctx);
int sa_ctx_strand_fold(sa_ctx *ctx, const int32_t *d_vfwd, const int32_t *d_vrev, const int32_t *d_sfwd, const int32_t *d_srev, int32_t nq,
		       int32_t *d_vbest, int32_t *d_sbest, uint64_t *d_bits, void *stream);
int sa_ctx_hits_strand(sa_ctx *ctx, const uint64_t *d_bits, int32_t nq, int32_t k, const int32_t *d_index, uint8_t *d_strand, void *stream);
int sa_ctx_hits_above_strand(sa_ctx *ctx, const uint64_t *d_bits, int32_t nq, const int64_t *d_offsets, const int32_t *d_index, uint8_t *d_strand,
			     void *stream);
bool sa_hip_search_strands(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp, int32_t k, int32_t *index,
			   int32_t *value, int32_t *score, uint8_t *strand, int32_t *rect, int32_t *vrect, uint8_t *srect, const struct sa_norm *norm,
			   const int32_t *pid_denom);
sa_hitlist *sa_hip_search_above_strands(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp,
					int32_t min_value, const struct sa_norm *norm, const int32_t *pid_denom);
const uint8_t *sa_hitlist_strand(const sa_hitlist *h);
double sa_hip_last_search_strands_seconds(void);

/* ---- alignments for chosen pairs: traceback on the device, run-length CIGARs ----------------------------------------
 * No reference counterpart: the reference keeps scores only.  For an explicit list of pairs (a[t], b[t]) of one store,
 * a != b, any order, duplicates allowed (the natural list: the N x k neighbours), the device repeats the exact s32 sweep of
 * the pair, records every cell's decision in scratch memory, walks the decisions back and returns one record and one CIGAR
 * per pair.
 *
 * CIGAR: uint32 runs, BAM style, len << 4 | op; SA_ALN_M: a residue of each sequence, SA_ALN_I: a residue of a only,
 * SA_ALN_D: a residue of b only.  Runs go from the start of the alignment to its end; adjacent runs differ in op.
 *
 * Orientation: the library computes in the reference's orientation -- lo = min(a, b) is the row sequence, hi = max(a, b) the
 * column sequence, the substitution matrix indexed as the score kernels index it -- so `score` equals the similarity-matrix
 * entry of the pair even for a matrix that is not symmetric.  For a > b the result is mirrored on output: I <-> D, spans
 * swapped.
 *
 * Tie rule (part of the contract; the same input gives the same bytes), canonical orientation: r indexes rows (lo),
 * c columns (hi); H / M, X (gap_x: from the left, consumes a residue of hi) and Y (gap_y: from above, consumes a residue
 * of lo) are the reference's tables, border cells included with the values src/bio/method/nw.c:14-20, ga.c:23-38 and
 * sw.c:18-30 give them.
 *   NW     start at (m, n).  At (r, c): r > 0 && c > 0 && H[r][c] == H[r-1][c-1] + S: diagonal; else r > 0 &&
 *          H[r][c] == H[r-1][c] + g: up; else left.  Stop at (0, 0).
 *   Gotoh  three states, start in M at (m, n).  M, not at the origin: r > 0 && c > 0 && M[r][c] == M[r-1][c-1] + S: diagonal;
 *          else M[r][c] == X[r][c]: enter state X at this cell; else enter state Y.  X at (r, c): emit a left step; then
 *          X[r][c] == M[r][c-1] + open: state M at (r, c-1) (open wins ties), else state X at (r, c-1).  Y: the same, upwards.
 *   SW     end cell: the cell with M == best of smallest r, then smallest c.  best == 0: the alignment is empty (cigar_len
 *          0, columns 0, all four span fields 0).  Otherwise walk as Gotoh, but in state M the first test is M[r][c] == 0:
 *          stop.  The spans are where the walk started and stopped.
 * (For every scoring a context accepts the border values leave no choice: along row 0 the walk goes left, along column 0
 * up; SW stops on a border.)
 *
 * What "the alignment has this score" means: the sum of S over the M columns plus, per gap run of length L, NW: L g;
 * Gotoh and SW: open + (L - 1) max(open, extend) -- the reference's recurrence lets a gap be re-opened from `match`, and
 * scorings with |open| < |extend| are accepted.  Adjacent I and D runs each pay their own open.
 *
 * Device memory: a pair needs one byte per cell of len_lo x 64 ceil(len_hi / 64) for the decisions; a call sorts its pairs
 * by that size and runs them in batches sized from the free device memory (SA_HIP_TRACE_BATCH_BYTES caps a batch).  Any
 * lengths the store accepts work.  A context runs one such call at a time, and not beside sa_ctx_align_range of the same
 * context (they share its strip-boundary scratch). */
enum { SA_ALN_M = 0, SA_ALN_I = 1, SA_ALN_D = 2 };
struct sa_aln {
	int32_t score;                  /* == the similarity-matrix entry of (a, b), always */
	int32_t a_begin, a_end;         /* half-open residue span of a covered by the alignment */
	int32_t b_begin, b_end;         /* same for b; NW / Gotoh: whole sequences */
	int32_t columns;                /* alignment length = sum of all run lengths */
	int32_t identities;             /* M columns whose two residue CODES (0..23) are equal */
	int32_t cigar_len;              /* number of runs */
	int64_t cigar_off;              /* first run in the flat cigar array: the sum of cigar_len of the pairs before this one */
};
typedef struct sa_alns sa_alns;   /* owns records + flat cigar in host memory */
/* on a context: host index arrays in, host result out.  NULL + sa_last_error for a == b, an index out of range,
 * npairs < 0; npairs == 0 gives a valid empty result. */
sa_alns *sa_ctx_alignments(sa_ctx *ctx, const int32_t *a, const int32_t *b, int64_t npairs);
/* one call: sa_ctx_create on the first device + sa_ctx_alignments.  NULL as well for a scoring the context refuses and
 * when there is no device. */
sa_alns *sa_hip_alignments(struct sa_input in, const struct sa_scoring *sc, const int32_t *a, const int32_t *b, int64_t npairs);
const struct sa_aln *sa_alns_records(const sa_alns *alns);          /* npairs records, in the caller's pair order */
const uint32_t *sa_alns_cigar(const sa_alns *alns, int64_t *runs);  /* flat runs; *runs (may be NULL) = their number */
int64_t sa_alns_count(const sa_alns *alns);                         /* npairs */
void sa_alns_destroy(sa_alns *alns);
/* device time (seconds) of the last successful sa_ctx_alignments / sa_hip_alignments call of this process: fill + walk */
double sa_hip_last_alignments_seconds(void);
/* ... and its parts: seconds of the fill kernels, of the walk (walk, scan of cigar_len, compaction), the DP cells filled
 * and the number of batches the call was cut into.  Any pointer may be NULL. */
void sa_hip_last_alignments_breakdown(double *fill_seconds, double *walk_seconds, int64_t *cells, int32_t *batches);

/* ---- score graph: every pair at or above a threshold, as CSR, built on the device -------------------------------------
 * No reference counterpart: the reference delivers the N x N matrix, and whoever clusters it (MCL, connected components /
 * single linkage, scipy.sparse.csgraph, networkx, igraph) thresholds every element on the host, usually to keep well under 1 %.
 * Contract: for a store of N sequences and an int32 min_score, entry (r, c) with c != r is an edge iff
 * score(r, c) >= min_score, score(r, c) the symmetric similarity-matrix entry; the diagonal is never a candidate; larger is
 * better for all three methods.  The result is the symmetric adjacency in CSR form:
 *   offsets  int64[N + 1]; offsets[0] = 0, offsets[r + 1] - offsets[r] = degree of r, offsets[N] = E (even: every undirected
 *            edge appears in both rows)
 *   index    int32[E]; row r's columns in ASCENDING c
 *   score    int32[E]; the score of each index entry
 * Any int32 threshold is valid: at or below the matrix minimum E = N (N - 1); above the maximum the result is valid and empty
 * (all offsets 0).  The order is part of the contract: the same store, scoring and threshold give the same bytes run after
 * run -- no position is decided by which workgroup or wave arrives first.  Offsets and every position computed from them are
 * 64-bit (N = 10^5 can give E near 10^10). */
/* device-resident, asynchronous on `stream`: d_packed = whole packed matrix of ctx's store; d_offsets: N + 1 int64 of device
 * memory.  Count and exclusive scan, no host synchronisation, no scratch memory. */
int sa_ctx_edge_offsets(sa_ctx *ctx, const int32_t *d_packed, int32_t min_score, int64_t *d_offsets, void *stream);
/* d_offsets as written by sa_ctx_edge_offsets for the SAME d_packed and min_score; d_index, d_score: offsets[N] int32 each.
 * The two calls are separate so that a device-resident caller can read offsets[N] and allocate exactly E elements. */
int sa_ctx_edge_fill(sa_ctx *ctx, const int32_t *d_packed, int32_t min_score, const int64_t *d_offsets,
		     int32_t *d_index, int32_t *d_score, void *stream);
typedef struct sa_edges sa_edges;   /* owns offsets / index / score in host memory, like sa_alns */
/* one call, host in / host out: align into device memory, count, read E (8 bytes), allocate 8 E bytes of device memory, fill,
 * copy back.  The matrix never leaves the device.  One device (the first).  NULL + sa_last_error (the message names N and E)
 * when the edges, or the packed matrix itself, do not fit; the process goes on working.  sa_hip_last_align_seconds() then
 * tells the device time of the alignment inside it. */
sa_edges *sa_hip_edges(struct sa_input in, const struct sa_scoring *sc, int32_t min_score);
/* on a tile job whose device holds the finished packed matrix: when sa_zjob_neighbors can answer, and refused in the same
 * cases (the walk is not finished; the matrix is dealt over several jobs; a d_full job). */
sa_edges *sa_zjob_edges(sa_zjob *job, int32_t min_score);
const int64_t *sa_edges_offsets(const sa_edges *e, int32_t *num);    /* num + 1 entries; *num (may be NULL) = N */
const int32_t *sa_edges_index(const sa_edges *e, int64_t *count);    /* *count (may be NULL) = E */
const int32_t *sa_edges_score(const sa_edges *e);
void sa_edges_destroy(sa_edges *e);
/* device time (seconds) of count + scan + fill in the last successful sa_hip_edges / sa_zjob_edges call */
double sa_hip_last_edges_seconds(void);

/* ---- single-linkage clustering: the whole dendrogram from one pass over the device matrix --------------------------------
 * No reference counterpart.  A CSR graph at one threshold answers one question; the single-linkage hierarchy of a similarity
 * matrix is its maximum spanning tree, N - 1 pairs, and cutting that tree at ANY score T leaves exactly the connected
 * components of the graph score >= T.  Built by Boruvka rounds over the device-resident packed triangle (csrc/sa_linkage.hip).
 * Total order (part of the contract): for pairs i < j with packed index p = j (j - 1) / 2 + i, pair e comes BEFORE pair f iff
 * score(e) > score(f), or the scores are equal and p(e) < p(f).  Under this strict order the maximum spanning tree of the
 * complete graph is unique: the same store and scoring give the same bytes run after run, for any matrix -- all scores equal
 * and the few distinct scores of SW on DNA included.
 *   pairs  int32[2 (N - 1)]; pairs[2 t] = lo < pairs[2 t + 1] = hi; the N - 1 tree pairs sorted by that order, best first: the
 *          order in which Kruskal's algorithm, and so single linkage, joins clusters
 *   score  int32[N - 1]; the score of each pair
 * Labels at a threshold (host only, from a tree): labels[r] = the smallest index in r's connected component of the graph
 * score >= T.  Any int32 T is valid: above the maximum labels[r] = r (N clusters), at or below the minimum all 0 (one cluster).
 * Merge table (host only, from a tree), in the convention of scipy.cluster.hierarchy: merge t joins clusters
 * left[t] < right[t]; ids below N are sequences, id N + u is the cluster made by merge u; size[t] = sequences in the new
 * cluster.  Turning scores into heights is left to the caller. */
size_t sa_linkage_scratch_bytes(int32_t num);          /* host only */
/* device-resident, asynchronous on `stream`, no host synchronisation, no allocation: d_packed = whole packed matrix of
 * ctx's store; d_pairs 2 (N - 1) int32, d_score N - 1 int32, d_scratch sa_linkage_scratch_bytes(N) bytes (8-byte aligned),
 * contents ignored.  ceil(log2 N) rounds are enqueued; the kernels of a round that finds one component return at once. */
int sa_ctx_linkage(sa_ctx *ctx, const int32_t *d_packed, int32_t *d_pairs, int32_t *d_score, void *d_scratch, void *stream);
typedef struct sa_linkage sa_linkage;                   /* owns pairs / score in host memory, like sa_edges */
/* one call, host in / host out: align into device memory, tree, copy back.  The matrix never leaves the device.  One device
 * (the first).  NULL + sa_last_error when the packed matrix does not fit; the process goes on working. */
sa_linkage *sa_hip_linkage(struct sa_input in, const struct sa_scoring *sc);
/* on a tile job whose device holds the finished packed matrix: when sa_zjob_edges can answer; refused in the same cases */
sa_linkage *sa_zjob_linkage(sa_zjob *job);
const int32_t *sa_linkage_pairs(const sa_linkage *l, int32_t *merges);   /* *merges (may be NULL) = N - 1 */
const int32_t *sa_linkage_score(const sa_linkage *l);
void sa_linkage_destroy(sa_linkage *l);
/* device time (seconds) of rounds + sort in the last successful sa_hip_linkage / sa_zjob_linkage call */
double sa_hip_last_linkage_seconds(void);
/* ... and the rounds of that call that found more than one component (<= ceil(log2 N)) */
int sa_hip_last_linkage_rounds(void);
/* host only, no device.  Both fail through sa_last_error with nothing written for a null argument and for a tree that is not
 * a tree (an index out of range, lo >= hi, a cycle); sa_linkage_labels also for scores that are not in the contract's order. */
/* returns the number of clusters, < 0 on a bad tree; labels: N int32 */
int32_t sa_linkage_labels(const int32_t *pairs, const int32_t *score, int32_t num, int32_t min_score, int32_t *labels);
/* left, right, size: N - 1 int32 each; 0 on success */
int sa_linkage_merges(const int32_t *pairs, int32_t num, int32_t *left, int32_t *right, int32_t *size);

/* ---- score distribution: exact order statistics of the matrix, selected on the device -------------------------------------
 * No reference counterpart.  --min-score and --clusters cut at a score T; a sensible T is a property of the score distribution
 * ("the best 1 % of the pairs"), and the scores are on the device when the alignment ends.
 * Contract: let s_0 <= s_1 <= ... <= s_{P-1} be the P = N (N - 1) / 2 entries of the packed triangle in ascending order, each
 * unordered pair once.  For a rank k, 0 <= k < P:
 *   value  int32: s_k
 *   below  int64: the number of pairs with score < s_k
 * So P - below pairs score at least value: sa_hip_edges with min_score = value gives E = 2 (P - below) edges, and cutting the
 * single-linkage tree at value leaves the components of exactly those pairs.
 * A call takes m ranks, 1 <= m <= SA_HIP_SELECT_MAX, in any order, duplicates allowed; results come back in the caller's order.
 * A rank outside [0, P), an m outside its range, N < 2 and a null pointer fail through sa_last_error with nothing written.  The
 * result is exact for any int32 contents, INT32_MIN and INT32_MAX included, and is the same bytes run after run: a radix select
 * (four passes over the matrix, csrc/sa_select.hip) whose only shared state are integer counts, which do not depend on which
 * workgroup or wave arrives first.
 * Fraction to rank (host only): sa_score_rank(pairs, q) = min(pairs - 1, (int64_t)floor(q * (double)pairs)) for 0 <= q <= 1, the
 * product being the plain IEEE double product (Python: min(P - 1, int(q * P))); q = 0 is the minimum, q = 1 the maximum;
 * -1 for a NaN, a q outside [0, 1] or pairs < 1. */
#define SA_HIP_SELECT_MAX 16
size_t  sa_select_scratch_bytes(int32_t m);                    /* host only; 0 for an m outside 1 .. SA_HIP_SELECT_MAX */
int64_t sa_score_rank(int64_t pairs, double q);                /* host only */
/* device-resident, asynchronous on `stream`, no host synchronisation, no allocation.  d_packed = whole packed matrix of
 * ctx's store (4-byte aligned: an offset view will do); ranks: HOST array (travels as kernel arguments); d_value m int32,
 * d_below m int64, d_scratch sa_select_scratch_bytes(m) bytes, 8-byte aligned, contents ignored */
int  sa_ctx_select(sa_ctx *ctx, const int32_t *d_packed, const int64_t *ranks, int32_t m,
		   int32_t *d_value, int64_t *d_below, void *d_scratch, void *stream);
/* host in / host out, one device (the first), the matrix never leaves it (as sa_hip_neighbors) */
bool sa_hip_select(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below);
/* on a finished tile job: answers when sa_zjob_edges can, refuses in the same cases with the same wording; 0 on success */
int  sa_zjob_select(sa_zjob *job, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below);
/* one alignment, then the cut and what it feeds, from the same device matrix.  A bad rank is refused before the alignment is
 * launched.  *min_score = the score at `rank`, the threshold of the returned graph; value / below as for sa_hip_select. */
sa_edges   *sa_hip_edges_at_rank(struct sa_input in, const struct sa_scoring *sc, int64_t rank, int32_t *min_score, int64_t *below);
sa_linkage *sa_hip_linkage_with_ranks(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m,
				      int32_t *value, int64_t *below);
double sa_hip_last_select_seconds(void);                       /* device time of the rounds of the last successful call */

/* ---- normalised scores: self-scores and a normalised triangle on the device ------------------------------------------------
 * No reference counterpart.  Raw scores grow with length: two unrelated long proteins outscore two identical short peptides, so
 * on a store of mixed lengths the neighbours, the graph, the tree and the order statistics above are led by the long sequences.
 * Clustering by similarity divides the score by the self-scores or by the lengths first.  Here that division happens where the
 * scores are: a normalised triangle in the same packed layout, which every consumer above reads unchanged.
 * Denominator d[k] of sequence k (norm.source):
 *   SA_NORM_SELF    the score the context's method and scoring give sequence k aligned with ITSELF: k is the row and the column
 *                   sequence, the table indexed exactly as for a pair (sa_scoring: NW [code of row][code of column], Gotoh and
 *                   SW [code of column][code of row] -- it matters for a table that is not symmetric), by the full DP; never
 *                   assumed to be the sum of the table's diagonal
 *   SA_NORM_LENGTH  meta[k].len
 * Value of the pair (i, j) with score s (norm.rule), all arithmetic exact and 64-bit:
 *   SA_NORM_MIN     D = min(d[i], d[j]),      num = s SA_NORM_SCALE
 *   SA_NORM_MAX     D = max(d[i], d[j]),      num = s SA_NORM_SCALE
 *   SA_NORM_MEAN    D = (int64) d[i] + d[j],  num = 2 s SA_NORM_SCALE
 *   D <= 0: INT32_MIN (an undefined ratio is the worst score for every consumer); otherwise floor(num / D), rounded towards
 *   MINUS INFINITY (Python's //; C's / truncates, and NW scores are often negative), saturated to [INT32_MIN, INT32_MAX].
 * A normalised score is in parts per million: 1000000 = "as good as the denominator".  Thresholds given to the consumers
 * (min_score of the graph, the cut of the tree) are then in parts per million too.  The same store, scoring and rule give the
 * same bytes run after run. */
enum { SA_NORM_SELF = 0, SA_NORM_LENGTH = 1 };               /* source of the per-sequence denominator d[k] */
enum { SA_NORM_MIN = 0, SA_NORM_MAX = 1, SA_NORM_MEAN = 2 }; /* how d[i] and d[j] combine                   */
#define SA_NORM_SCALE 1000000                                /* a normalised score is in parts per million  */
struct sa_norm {
	int32_t source;        /* SA_NORM_SELF / SA_NORM_LENGTH */
	int32_t rule;          /* SA_NORM_MIN / SA_NORM_MAX / SA_NORM_MEAN */
	int32_t *denominators; /* out, host, N int32: receives d[0 .. N); may be NULL */
};
/* host only: the value rule above for one entry.  INT32_MIN + sa_last_error for a rule outside the enum. */
int32_t sa_norm_value(int32_t s, int32_t di, int32_t dj, int32_t rule);
/* device-resident, asynchronous on `stream`: d_den = N int32 of device memory (on a search context: the N + M of the
 * concatenated store, database first).  SA_NORM_SELF runs one wavefront per sequence
 * over the context's strip-boundary scratch, so -- like sa_ctx_alignments -- it does not run beside sa_ctx_align_range (or
 * another sa_ctx_denominators) of the SAME context on another stream; in order on one stream is fine.  SA_NORM_LENGTH copies
 * the lengths.  Non-zero + sa_last_error for a null pointer or a source outside the enum, nothing launched. */
int sa_ctx_denominators(sa_ctx *ctx, int32_t source, int32_t *d_den, void *stream);
/* device-resident, asynchronous on `stream`, no scratch memory, no host synchronisation: d_out[p] = value of d_packed[p] for
 * the whole packed matrix of ctx's store.  d_den: ANY N int32 of device memory -- sa_ctx_denominators' or the caller's own.
 * d_packed / d_out need their natural 4-byte alignment only (an offset view will do); d_out == d_packed (in place) and
 * disjoint buffers are both valid, partial overlap is not. */
int sa_ctx_normalize(sa_ctx *ctx, const int32_t *d_packed, const int32_t *d_den, int32_t rule, int32_t *d_out, void *stream);
/* on a sa_hip_tiles_begin job whose device holds the whole finished matrix (after sa_zjob_next has returned 0): normalises the
 * job's matrix IN PLACE, once; sa_zjob_neighbors / _edges / _linkage / _select then answer over normalised scores.  The tiles
 * already handed out stay raw.  Refused, in the wording of sa_zjob_edges: before the walk is finished, a second call, a
 * sa_zjob_create job (its matrix is the caller's, and const), several devices, SA_HIP_TILES_SPLIT > 1, a d_full job. */
int sa_zjob_normalize(sa_zjob *job, const struct sa_norm *norm);
/* the one-call variants: the arguments of the namesake + norm.  norm == NULL: exactly the namesake.  Otherwise denominators and
 * sweep follow the alignment on its stream, in place, and the selection reads normalised scores; norm->denominators, when not
 * NULL, receives d[0 .. N) on success.  A source or rule outside its enum is refused before the alignment is launched. */
bool sa_hip_neighbors_norm(struct sa_input in, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score, const struct sa_norm *norm);
sa_edges *sa_hip_edges_norm(struct sa_input in, const struct sa_scoring *sc, int32_t min_score, const struct sa_norm *norm);
sa_linkage *sa_hip_linkage_norm(struct sa_input in, const struct sa_scoring *sc, const struct sa_norm *norm);
bool sa_hip_select_norm(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below,
			const struct sa_norm *norm);
sa_edges *sa_hip_edges_at_rank_norm(struct sa_input in, const struct sa_scoring *sc, int64_t rank, int32_t *min_score, int64_t *below,
				    const struct sa_norm *norm);
sa_linkage *sa_hip_linkage_with_ranks_norm(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m,
					   int32_t *value, int64_t *below, const struct sa_norm *norm);
/* device time (seconds) of denominators + sweep in the last successful *_norm / sa_zjob_normalize call */
double sa_hip_last_normalize_seconds(void);

/* ---- percent identity of every pair: identities and columns carried through the sweep ----------------------------------------
 * No reference counterpart.  The number biologists cut at is percent identity ("cluster at 90 % identity"); the -f filter knows
 * only the positional identity of unaligned prefixes, and sa_ctx_alignments costs a decision byte per DP cell plus a walk per
 * chosen pair.  Here every pair of the store gets the `identities` and `columns` of its canonical alignment -- the ONE alignment
 * the tie rule of "alignments for chosen pairs" above fixes, the same two numbers struct sa_aln reports -- from one forward
 * sweep: the canonical path is a per-cell function of the DP tables, so both numbers travel with the scores (csrc/sa_identity.hip,
 * csrc/sa_identity_core.h).  No decision scratch, no walk.
 * Everything is in the canonical orientation: pair i < j, i the row sequence; the score is the similarity-matrix entry, always,
 * and nothing depends on the order in which a caller names the two sequences.  An empty SW alignment (best == 0) has
 * identities = columns = 0.
 * Percent identity in parts per million (pid), exact 64-bit arithmetic, from identities, columns and the two lengths:
 *   SA_PID_COLUMNS   D = columns,             num = identities SA_NORM_SCALE
 *   SA_PID_SHORTER   D = min(len_i, len_j),   num = identities SA_NORM_SCALE
 *   SA_PID_LONGER    D = max(len_i, len_j),   num = identities SA_NORM_SCALE
 *   SA_PID_MEAN      D = len_i + len_j,       num = 2 identities SA_NORM_SCALE
 *   D <= 0: INT32_MIN, as sa_norm_value (only an empty SW alignment under SA_PID_COLUMNS gets there); otherwise floor(num / D),
 *   in [0, 1000000].
 * A triangle of pid is a packed triangle like any other: the neighbours, the graph, the tree and the order statistics above read
 * it unchanged, and their thresholds are then in parts per million.  The same store and scoring give the same bytes run after run. */
enum { SA_PID_COLUMNS = 0, SA_PID_SHORTER = 1, SA_PID_LONGER = 2, SA_PID_MEAN = 3 };
struct sa_identity_out {
	int32_t *score, *identities, *columns, *pid; /* any subset non-NULL; element [p - start] belongs to pair p */
	int32_t denom;                               /* SA_PID_*; read iff pid != NULL */
};
/* host only: the value rule above for one pair.  INT32_MIN + sa_last_error for a denom outside the enum. */
int32_t sa_pid_value(int32_t identities, int32_t columns, int32_t len_i, int32_t len_j, int32_t denom);
/* device-resident, asynchronous on `stream`: the packed pair range [start, start + count) into the DEVICE arrays of *d_out (the
 * struct itself is host memory).  Any two outputs may not overlap; an output may be a buffer that held something else -- the
 * kernel reads none of them, so pid can replace a triangle of scores in place.  One wavefront per pair over the context's
 * strip-boundary scratch plus a buffer of boundary payloads the context allocates at its first identity call (twice the bytes
 * of that scratch): like sa_ctx_alignments, the call does not run beside sa_ctx_align_range or another identity call of the SAME
 * context on another stream; in order on one stream is fine.  Non-zero + sa_last_error, nothing launched, for a null argument,
 * all four outputs NULL, a denom outside the enum (when pid is asked for), a range outside [0, pairs). */
int sa_ctx_identity_range(sa_ctx *ctx, int64_t start, int64_t count, const struct sa_identity_out *d_out, void *stream);
/* host in / host out, one device (the first): identities, columns, pid are HOST packed triangles (N (N - 1) / 2 int32 each), any
 * subset non-NULL; denom is read iff pid != NULL.  Runs in column-aligned ranges sized from the free device memory
 * (SA_HIP_IDENTITY_BATCH_BYTES caps a range), so any N whose triangles fit the host works.  The arguments are checked before a
 * device is looked for. */
bool sa_hip_identity(struct sa_input in, const struct sa_scoring *sc, int32_t denom, int32_t *identities, int32_t *columns, int32_t *pid);
/* on a sa_hip_tiles_begin job whose device holds the whole finished matrix: overwrites the job's matrix with pid IN PLACE, once;
 * sa_zjob_neighbors / _edges / _linkage / _select then answer over percent identity.  The tiles already handed out stay raw.
 * Refused when sa_zjob_normalize is, with the same wording; also after sa_zjob_normalize, and sa_zjob_normalize after it. */
int sa_zjob_identity(sa_zjob *job, int32_t denom);
/* the one-call selections over percent identity: the arguments of the namesake + denom.  The identity sweep fills the device
 * triangle with pid; no score alignment runs.  Null arguments, a bad denom, a bad k / rank are refused before a device is
 * looked for. */
bool sa_hip_neighbors_pid(struct sa_input in, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score, int32_t denom);
sa_edges *sa_hip_edges_pid(struct sa_input in, const struct sa_scoring *sc, int32_t min_score, int32_t denom);
sa_linkage *sa_hip_linkage_pid(struct sa_input in, const struct sa_scoring *sc, int32_t denom);
bool sa_hip_select_pid(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below,
		       int32_t denom);
sa_edges *sa_hip_edges_at_rank_pid(struct sa_input in, const struct sa_scoring *sc, int64_t rank, int32_t *min_score, int64_t *below,
				   int32_t denom);
sa_linkage *sa_hip_linkage_with_ranks_pid(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m,
					  int32_t *value, int64_t *below, int32_t denom);
/* device time (seconds) of the identity sweep in the last successful sa_hip_identity / *_pid / sa_zjob_identity call */
double sa_hip_last_identity_seconds(void);

/* ---- queries fitted inside database sequences: the whole query, the database's overhang free ----------------------------------
 * No reference counterpart.  What a search asks -- a read against a database entry, a domain against a full-length protein -- is
 * the WHOLE query placed anywhere inside the database sequence: "fit", "glocal" or semi-global alignment.  NW and Gotoh charge the
 * query for every database residue that overhangs it; SW may drop the ends of the query.  Here the query's ends are fixed and the
 * database's are free, and the call also says where in the database sequence the query sits.
 * Orientation: canonical, as everywhere on a search context.  The database sequence d (length m) is the row sequence, r = 0 .. m;
 *   the query (length n) is the column sequence, c = 0 .. n.  The substitution table is indexed as struct sa_scoring documents for
 *   the method.
 * Methods: SA_METHOD_NW (linear gap g) and SA_METHOD_GA (open o, extend e).  SA_METHOD_SW is refused: it is already local.
 * Tables: the reference's recurrences for the method, unchanged (nw.c:29-35, ga.c:46-63).  Row 0 is the method's: M[0][c] =
 *   border(c), Y[0][c] = SCORE_MIN.  The one difference: M[r][0] = 0 for every r = 0 .. m (X[r][0] = SCORE_MIN as before) --
 *   leaving the database's first residues costs nothing.
 * End cell: among the cells (r, n), r = 0 .. m, the one with the largest M, on a tie the smallest r.  score = M there, db_end = r.
 *   Row 0 takes part: M[0][n] = border(n), the query against nothing.
 * Walk: start in state M at (db_end, n); the records are those of the alignment contract above, so the tie rule exists once.
 *   At c == 0: stop, db_begin = r there.  At r == 0, c > 0: one step left.  Elsewhere: as the alignment contract walks the method.
 * Spans: the query's is always [0, n); the database's is [db_begin, db_end), 0 <= db_begin <= db_end <= m.
 * identities, columns: of that walk, as struct sa_aln counts them; they travel forward with the scores together with db_begin
 *   (csrc/sa_fit.hip, csrc/sa_fit_core.h): payload borders P(r, 0) = (0, 0, r), P(0, c) = (0, c, 0); no decision scratch, no walk.
 *   pid is the value rule of "percent identity of every pair" over (identities, columns, m, n).
 * What the score means: the best global score of the query against any substring d[s, e), 0 <= s <= e <= m; the empty substring
 *   counts and gives border(n).  Hence NW / Gotoh score <= fit score, and under Gotoh fit score <= the SW score of the same gaps.
 * The rectangle of fit scores is a dense rect[q * N + d] like that of sa_ctx_search_range: sa_ctx_hits, sa_ctx_hits_above_*,
 * sa_ctx_normalize_rect and sa_ctx_strand_fold read it unchanged.  The same input gives the same bytes run after run. */
struct sa_fit_out {
	int32_t *score, *db_begin, *db_end, *identities, *columns, *pid; /* any subset non-NULL */
	int32_t denom;                                                   /* SA_PID_*; read iff pid != NULL */
};
/* device-resident, asynchronous on `stream`, search contexts only (a strands context is one: its rows M .. 2 M are the reverse
 * complements): queries [q0, q0 + nq) against every database sequence into the DEVICE arrays of *d_out (the struct itself is host
 * memory), nq * N int32 each, element (q - q0) * N + d.  One wavefront per pair over the context's strip-boundary scratch plus the
 * boundary payloads the context allocates at its first fit call -- the identity sweep's buffer (twice the bytes of that scratch,
 * shared with it) and one of its own for the third payload word (once its bytes) -- and never afterwards: the rule of sa_ctx_alignments applies -- not beside sa_ctx_align_range / sa_ctx_search_range or another sweep of the
 * SAME context on another stream; in order on one stream is fine.  Non-zero + sa_last_error, nothing launched, for a null
 * argument, an ordinary context, a context whose method is SW, every output NULL, a denom outside the enum (when pid is asked
 * for), q0 / nq out of range. */
int sa_ctx_fit_rect(sa_ctx *ctx, int32_t q0, int32_t nq, const struct sa_fit_out *d_out, void *stream);
/* the list form: item w is the query d_query[w] (0 .. the context's queries - 1) against the database sequence d_db[w]
 * (0 .. N - 1), both DEVICE int32 arrays of npairs entries read by the kernel in stream order, element w of every non-NULL output;
 * any order, duplicates allowed (the natural list: the nq x k hits).  An index outside its range reads nothing and gives
 * INT32_MIN in every output asked for.  npairs == 0 launches nothing.  Refusals as above, and npairs < 0. */
int sa_ctx_fit_pairs(sa_ctx *ctx, const int32_t *d_query, const int32_t *d_db, int64_t npairs, const struct sa_fit_out *d_out,
		     void *stream);
/* the fitted alignments of chosen pairs, as sa_ctx_alignments returns alignments: HOST index arrays in (query[t] in [0, the
 * context's queries), db[t] in [0, N)), host result out, one record and one CIGAR per pair in the caller's order.  The fill and
 * the walk are those of "alignments for chosen pairs" with the fit borders, end cell and walk step; batching, scan and compaction
 * are shared (SA_HIP_TRACE_BATCH_BYTES caps a batch; sa_hip_last_alignments_seconds / _breakdown report the call).  Record
 * layout, with a = the query and b = the database sequence: a_begin = 0, a_end = n; b_begin = db_begin, b_end = db_end; SA_ALN_I
 * is a residue of the query only, SA_ALN_D of the database sequence only; score, columns and identities are those of
 * sa_ctx_fit_pairs for the pair.  The CIGAR scores `score` as the alignment contract prices an alignment.  NULL + sa_last_error
 * for an ordinary context, SW, an index out of range, npairs < 0; npairs == 0 gives a valid empty result. */
sa_alns *sa_ctx_fit_alignments(sa_ctx *ctx, const int32_t *query, const int32_t *db, int64_t npairs);
/* host in / host out, one device (the first): the fit search.  index, value, score, db_begin, db_end are (M, k) HOST arrays, rect
 * and vrect (M, N), as sa_hip_search_pid lays them out; value, score, db_begin, db_end belong to the hits of index.  denom == -1:
 * the hits are ranked by the fit score (value, when asked for, is a copy of score; vrect of rect); denom = SA_PID_*: by the
 * percent identity of the fitted alignment.  Ties: index ascending.  Per batch of queries the rectangle sweep gives the score
 * (and pid), sa_ctx_hits selects, and the list form over the nq x k hits gives db_begin / db_end and the raw score: no begin or
 * end rectangle is ever made.  Batches are sized from the free device memory (SA_HIP_SEARCH_BATCH_BYTES caps a batch; a query
 * costs 8 N + 32 k bytes).  The arguments are checked before a device is looked for: null arguments, SW, a denom that is neither
 * -1 nor in the enum, a bad k, empty stores. */
bool sa_hip_search_fit(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t denom,
		       int32_t *index, int32_t *value, int32_t *score, int32_t *db_begin, int32_t *db_end, int32_t *rect, int32_t *vrect);
/* device time (seconds) of the fit sweeps -- rectangle and list -- summed over the batches of the last successful sa_hip_search_fit */
double sa_hip_last_search_fit_seconds(void);

/* ---- complete and average linkage: the two other hierarchies of the device matrix ------------------------------------------
 * No reference counterpart.  The flat clusters of single linkage are connected components, and on protein families connected
 * components chain: one bridging sequence joins two unrelated groups.  Complete linkage promises that EVERY pair inside a
 * cluster scores at least T; average linkage (UPGMA) is the classical guide tree.  Both need the whole matrix between merges,
 * not a spanning tree -- and the whole matrix is on the device when the alignment ends (csrc/sa_agglo.hip).
 * Input: the packed triangle of N sequences, pair i < j at p(i, j) = j (j - 1) / 2 + i, int32, any contents.  Method:
 * SA_AGGLO_COMPLETE or SA_AGGLO_AVERAGE; 0 is reserved for single linkage and refused here (sa_ctx_linkage builds it).
 * Clusters: a cluster is named by its smallest member; at first every sequence is a cluster.
 * Similarity of two clusters A, B:
 *   complete  the minimum of score(a, b) over a in A, b in B (int32)
 *   average   the exact rational S(A, B) / (|A| |B|), S the int64 sum of those scores; no floating point anywhere
 * Total order (part of the contract; the single-linkage order lifted to clusters): cluster pair e = (A, B) with names a < b has
 * p(e) = b (b - 1) / 2 + a; e comes BEFORE f iff sim(e) > sim(f), or the similarities are equal and p(e) < p(f).  Two averages
 * are equal iff S1 n2 == S2 n1 in 128 bits.
 * Step t = 0 .. N - 2: the first pair in that order among all pairs of active clusters is merged; the union keeps the name a;
 * its similarity to every other cluster C is min(sim(A, C), sim(B, C)) (complete) or S(A, C) + S(B, C) with size |A| + |B|
 * (average).
 *   pairs  int32[2 (N - 1)]; pairs[2 t] = a < pairs[2 t + 1] = b, in the order the merges are made
 *   score  int32[N - 1]; complete: the minimum; average: floor(S / (|A| |B|)), rounded towards minus infinity as sa_norm_value
 * The shape of the single-linkage tree: sa_linkage_pairs, sa_linkage_score, sa_linkage_destroy and sa_linkage_merges serve
 * unchanged.  score is non-increasing (the floors of the averages too), and the pairs form a spanning tree with lo < hi; so
 * sa_linkage_merges gives the merge table in scipy's convention, and for an integer T "merged at similarity >= T" is
 * score[t] >= T.  Equal scores need NOT be in ascending p, so sa_linkage_labels may rightly refuse such a tree;
 * sa_agglo_labels reads it.  On a matrix without ties the merge table and the heights equal
 * scipy.cluster.hierarchy.linkage(-scores, 'complete' | 'average').
 * Range: average needs |S| <= 2^31 N^2 / 4 inside int64, so N <= 131072; complete N <= 2^30; a larger N is refused before
 * anything is launched.  "No candidate" is never a score value: INT32_MIN and INT32_MAX are scores.  The same store, scoring
 * and method give the same bytes run after run. */
#define SA_AGGLO_COMPLETE 1
#define SA_AGGLO_AVERAGE 2
/* host only: the scratch memory sa_ctx_agglomerate needs -- the square working matrix, 4 N^2 + O(N) bytes (complete) or
 * 8 N^2 + O(N) (average); 0 for a bad method, num < 2 or an N outside the method's range */
size_t sa_agglo_scratch_bytes(int32_t num, int32_t method);
/* device-resident, asynchronous on `stream`, no host synchronisation, no allocation: d_packed = whole packed matrix of ctx's
 * store, read only; d_pairs 2 (N - 1) int32, d_score N - 1 int32, d_scratch sa_agglo_scratch_bytes(N, method) bytes (8-byte
 * aligned), contents ignored.  2 N launches are enqueued: two small kernels per merge. */
int sa_ctx_agglomerate(sa_ctx *ctx, const int32_t *d_packed, int32_t method, int32_t *d_pairs, int32_t *d_score, void *d_scratch,
		       void *stream);
/* one call, host in / host out, one device (the first): align into device memory, tree, copy back.  norm and pid_denom both
 * NULL: the scores; norm: the normalised scores, as sa_hip_linkage_norm; pid_denom: percent identity under *pid_denom, as
 * sa_hip_linkage_pid; both: refused.  A bad method, both quantities and an N out of range are refused before a device is
 * looked for.  NULL + sa_last_error, naming the bytes needed, when matrix + scratch do not fit; the process goes on working. */
sa_linkage *sa_hip_agglomerate(struct sa_input in, const struct sa_scoring *sc, int32_t method, const struct sa_norm *norm,
			       const int32_t *pid_denom);
/* one alignment, the order statistics and the tree from the same device matrix, as sa_hip_linkage_with_ranks; a bad rank is
 * refused before the alignment */
sa_linkage *sa_hip_agglomerate_with_ranks(struct sa_input in, const struct sa_scoring *sc, int32_t method, const struct sa_norm *norm,
					  const int32_t *pid_denom, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below);
/* on a finished tile job: answers when sa_zjob_linkage can, refuses in the same cases with the same wording */
sa_linkage *sa_zjob_agglomerate(sa_zjob *job, int32_t method);
/* host only, no device: applies the merges t with score[t] >= min_score (a prefix); labels[r] = the smallest index in r's
 * cluster; returns the number of clusters.  < 0 through sa_last_error with nothing written for a null argument, pairs that are
 * not a tree (an index out of range, lo >= hi, a cycle) and scores that increase. */
int32_t sa_agglo_labels(const int32_t *pairs, const int32_t *score, int32_t num, int32_t min_score, int32_t *labels);
/* device time (seconds) of the last successful sa_hip_agglomerate* / sa_zjob_agglomerate call */
double sa_hip_last_agglomerate_seconds(void);
/* ... and the rows that call scanned again after a merge took their cached partner (a diagnostic; 0 on an all-equal matrix) */
int64_t sa_hip_last_agglomerate_rescans(void);

/* ---- pair-space planning (host only, no device needed) -------------------
 * DP cells (sum of len_i*len_j) of the packed pair range [start, start+count),
 * the numerator of GCUPS; -1 on a bad range. */
int64_t sa_pairs_cells(const struct sa_meta *meta, int32_t num, int64_t start, int64_t count);
/* Splits [0, N(N-1)/2) into `parts` contiguous ranges of near-equal DP work
 * (cells); bounds[parts+1] receives the cut points (bounds[0]=0,
 * bounds[parts]=pairs).  Multi-GPU sharding rule, SURVEY.md §8(e): the
 * reference's own batch abstraction kernel(scores, start, batch) is a range. */
int sa_pairs_partition(const struct sa_meta *meta, int32_t num, int parts, int64_t *bounds);

/* Instrumentation for bench.py.  While enabled every kernel launch of
 * sa_ctx_align_range is bracketed by a HIP-event pair on the launch stream.
 * sa_ctx_timing_read reports the DOMINANT kernel (largest accumulated time)
 * since the last enable: its name, launch count, accumulated milliseconds and
 * the pairs / DP cells those launches covered, plus the sum over all kernels. */
void sa_ctx_timing(sa_ctx *ctx, int enable);
int sa_ctx_timing_read(sa_ctx *ctx, char *kernel_name, int cap, int64_t *launches, double *total_ms,
		       int64_t *pairs, int64_t *cells, double *all_kernels_ms);

/* ---- option tables (host only, no device needed) ------------------------ */

/* Replaces parse_matrix (src/bio/matrices.c:44-58): case-insensitive name ->
 * SEQ_LUT + SUB_MAT.  0 on success. */
int sa_matrix_load(const char *name, int32_t lut[SA_LUT_SIZE], int32_t sub[SA_SUB_DIM * SA_SUB_DIM]);
/* -l / list_matrices (src/bio/matrices.c:27-33) */
int sa_matrix_count(void);
const char *sa_matrix_name(int index);
int sa_matrix_is_nucleotide(int index);

/* Replaces parse_align (src/bio/align.c:87-96): alias ("nw", "Needleman-Wunsch",
 * ... case-insensitive) -> enum sa_method, -1 if unknown. */
int sa_method_parse(const char *alias);
const char *sa_method_name(int method);   /* long alias, e.g. "Gotoh"       */
int sa_method_gap_kind(int method);       /* enum sa_gap_kind               */

/* ---- misc ---------------------------------------------------------------- */
/* Seconds the launch/copy loop of the last successful sa_hip_align() took (after sa_hip_neighbors: the device time of
 * its alignment): the phase the reference
 * brackets with bench_align_start()/bench_align_end() (src/interface/seqalign_cuda.c:182,292 --
 * uploads, allocations and context set-up are outside it, the device->host copies inside). */
double sa_hip_last_align_seconds(void);
/* Which schedule the last successful sa_hip_align() took: 1 = every device delivers a contiguous slice of the packed
 * index straight into the host matrix (one device: the whole range); 2 = tile-interleaved dense shares + RCCL
 * all-gather + placement on every device, then delivery (several devices); 0 = no call yet. */
int sa_hip_last_align_path(void);

/* Progress of a running sa_hip_align / sa_ctx_align_host, the reference's ppercent / pproportc side channel
 * (src/interface/seqalign_cuda.c:181,286-289,293): fn(fraction in [0,1], user) is called while the host waits for the
 * device -- per batch on the batched paths, every 50 ms from the launches' tile counters on the single-launch path --
 * from the calling thread when one device is used, from ONE worker thread of the library (the first slice's) when
 * sa_hip_align spreads the job over several: calls never overlap, but the callback must not assume the caller's thread.
 * NULL (the default) reports nothing and polls nothing; the polling waits in 250 us slices and never past completion. */
typedef void (*sa_progress_fn)(double fraction, void *user);
void sa_hip_set_progress(sa_progress_fn fn, void *user);

/* Where the time of the last successful sa_hip_align() went, in milliseconds (its first slice): ms[k] for k of
 * enum sa_breakdown; returns the number of entries written.  Everything but SA_BREAKDOWN_PHASE is set-up the reference
 * keeps outside bench_align_start()/bench_align_end() as well (src/interface/seqalign_cuda.c:115-168). */
enum sa_breakdown {
	SA_BREAKDOWN_ENCODE = 0,   /* validate + residue -> index (the reference uploads SEQ_LUT instead)        */
	SA_BREAKDOWN_DEVICE,       /* hipSetDevice / runtime bring-up                                            */
	SA_BREAKDOWN_UPLOAD,       /* device allocations, uploads, streams and events                            */
	SA_BREAKDOWN_CODE_OBJECTS, /* loading the kernel families this store needs                               */
	SA_BREAKDOWN_PIN,          /* page-locking the destination (skipped when the caller registered it)       */
	SA_BREAKDOWN_PLAN,         /* launch plan of the range (tile lists)                                      */
	SA_BREAKDOWN_ARRANGE,      /* arranged copies of the row store                                           */
	SA_BREAKDOWN_PHASE,        /* the launch/copy loop = sa_hip_last_align_seconds()                         */
	SA_BREAKDOWN_TOTAL,        /* create + align_host of the slice                                           */
	SA_BREAKDOWN_COUNT
};
int sa_hip_last_align_breakdown(double *ms, int n);

int sa_hip_device_count(void);
const char *sa_hip_device_name(int device);
const char *sa_last_error(void);
int sa_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SEQALIGN_HIP_H */
