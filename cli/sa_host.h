/*
 * cli/sa_host.h -- host side of the `seqalign` command line tool (plain C, no device code).
 *
 * Mirrors the reference's input/output layer around the device boundary:
 *   sa_host_load      <- input_load        src/io/input.c:28-93  (+ parsers src/io/source/{fasta,dsv}.c)
 *   sa_host_filter    <- filter            src/bio/filter.c:14-89 (sequential semantics)
 *   sa_host_matrix_*  <- output_load/free  src/io/output.c:16-66,101-106
 *   sa_host_write_hdf5<- flush_hdf5        src/io/format/hdf5.c:14-202
 * Everything returns 0 on success and leaves a message in sa_host_error() otherwise.
 */
#ifndef SA_HOST_H
#define SA_HOST_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "../include/seqalign_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *sa_host_error(void);

/* The reference's `struct input` plus ownership (io/input.h:6-11). */
struct sa_host_store {
	struct sa_input in; /* seqs: NUL-separated uppercase blob, meta[k] = {off,len} */
	size_t blob_bytes;
};

/* Parse a whole file image already in memory (used by tests) or a file on disk.
 * `ext` selects the parser like the reference does (extension without the dot):
 * fasta fa fas fna ffn faa frn mpfa | csv tsv ssv psv.  `lut` is SEQ_LUT (residue validation,
 * fasta.c:57-63).  DSV: the sequence column is found by header name (dsv.c:21-24); when no
 * header matches, `dsv_column` (0-based) is used if >= 0, with `dsv_has_header` telling whether
 * the first row is a header -- the non-interactive form of the reference's prompt (dsv.c:128-151);
 * -1 makes that situation an error. */
int sa_host_parse(const uint8_t *data, size_t size, const char *ext, const int32_t lut[SA_LUT_SIZE],
		  int32_t gap_for_length_limit, int dsv_column, int dsv_has_header, struct sa_host_store *out);
int sa_host_load(const char *path, const int32_t lut[SA_LUT_SIZE], int32_t gap_for_length_limit,
		 int dsv_column, int dsv_has_header, struct sa_host_store *out);
void sa_host_store_free(struct sa_host_store *s);

/* -f threshold: for j ascending drop j if some KEPT i<j has matches(first min(len))/min(len) >= thr;
 * compacts blob + meta in place (filter.c:66-79).  Returns kept count (<0 on error). */
int32_t sa_host_filter(struct sa_host_store *s, float threshold, int threads);

/* Compacts blob + meta in place keeping the sequences with keep[k] != 0 (filter.c:66-79); returns the
 * number kept (<0 when fewer than 2 remain). */
int32_t sa_host_compact(struct sa_host_store *s, const uint8_t *keep);

/* Result matrix (output.c:16-66, os.c:32-141): zero-filled mapping of 4*N*N or 4*N(N-1)/2 bytes -- anonymous, or of an
 * unnamed temporary file when `file_backed` (what the reference does once the full matrix exceeds 3/4 of
 * MemAvailable, sa_host_matrix_needs_file; it then also stores the matrix triangular). */
int32_t *sa_host_matrix_alloc(size_t num, bool triangular, bool file_backed);
void sa_host_matrix_free(int32_t *m, size_t num, bool triangular);
size_t sa_host_available_memory(void); /* MemAvailable, os.c:262-295; SA_HOST_MEM_AVAILABLE=<bytes> overrides (tests) */
bool sa_host_matrix_needs_file(size_t num);

/* HDF5: /sequences (N vlen C strings) + /similarity_matrix (N x N I32LE, symmetric, zero diagonal);
 * chunked only when N > 256, chunk = clamp(largest 64*2^k <= N, 256, 4096), deflate level z on the
 * chunked dataset; libver latest, 4 KiB alignment (hdf5.c:16-18,70-89).  A packed triangular matrix
 * is expanded in row blocks (diagonal written as 0). */
int sa_host_write_hdf5(const char *path, const struct sa_host_store *s, const int32_t *matrix, bool triangular,
		       unsigned compression);
size_t sa_host_hdf5_chunk_dim(size_t dim); /* exposed for tests */
/* ... and the same file from tiles that arrive finished -- zlib streams from the device-side encoder of the -z option, or
 * (compression 0) the raw tiles; include/seqalign_hip.h: sa_zjob_next has exactly this signature:
 * next(user, rows, cols, streams, sizes) fills the next batch of at most ceil(N / chunk) tiles (tile coordinates + bytes,
 * valid until its next call) and returns their number, 0 at the end, < 0 on error; the tiles go to H5Dwrite_chunk unchanged,
 * in whatever order they come. */
typedef int (*sa_host_tiles_fn)(void *user, uint32_t *rows, uint32_t *cols, const uint8_t **streams, size_t *sizes);
int sa_host_write_hdf5_streams(const char *path, const struct sa_host_store *s, unsigned compression, sa_host_tiles_fn next,
			       void *user);
/* The -k option: /neighbor_indices and /neighbor_scores, N x k I32LE each, contiguous (the arrays of sa_hip_neighbors /
 * sa_zjob_neighbors).  create = 0 reopens the finished file at `path` and adds the two datasets; create = 1 writes a new
 * file with /sequences and the two, no /similarity_matrix (--neighbors-only). */
int sa_host_write_neighbors(const char *path, const struct sa_host_store *s, int32_t k, const int32_t *index, const int32_t *score,
			    int create);
/* --alignments: /neighbor_alignment_records (N x k x 8 int32: the fields of struct sa_aln up to cigar_len),
 * /neighbor_cigar_offsets (N k + 1 int64: entry t = cigar_off of record t, row-major; the last = `runs`) and
 * /neighbor_cigars (`runs` uint32), added to the file at `path` (which sa_host_write_neighbors has written to). */
int sa_host_write_alignments(const char *path, const struct sa_host_store *s, int32_t k, const struct sa_aln *records,
			     const uint32_t *cigar, int64_t runs);
/* --query: the one writer of a search.  A NEW file at `path` with /sequences (the database as searched, N), /query_sequences (M),
 * /hit_indices and /hit_scores (M x k I32LE, the arrays of sa_hip_search: row q lists the k best database sequences of query q,
 * indices into /sequences); with `rect` (or NULL) also /query_scores (M x N I32LE, rect[q * N + d]); with `records` (or NULL) also
 * /hit_alignment_records (M x k x 8), /hit_cigar_offsets (M k + 1 I64LE) and /hit_cigars (`runs` U32LE), in the format of the
 * neighbour datasets (a = the query, b = its hit).  No /similarity_matrix.  k outside [1, min(N, 64)] or an index outside [0, N)
 * give an error before anything is opened; a file that fails later is removed. */
int sa_host_write_search(const char *path, const struct sa_host_store *db, const struct sa_host_store *queries, int32_t k,
			 const int32_t *index, const int32_t *score, const int32_t *rect, const struct sa_aln *records, const uint32_t *cigar,
			 int64_t runs);
/* --query --hits-by: the values the hits were ranked by, ADDED to the finished file of sa_host_write_search at `path`, whose other
 * datasets stay as they are: /hit_values (M x k I32LE, parts per million; row q descending, ties by index ascending), /hit_quantity
 * (3 I32LE: kind 1 = normalised score, 2 = percent identity; source, SA_NORM_SELF / SA_NORM_LENGTH, or 0; rule, SA_NORM_MIN / _MAX /
 * _MEAN, or the denominator SA_PID_*), /hit_scale (1 I32LE: SA_NORM_SCALE); kind 1 with `denominators` (N + M, database first) also
 * /database_denominators (N) and /query_denominators (M); with `vrect` (or NULL) also /query_values (M x N I32LE).  The arguments are
 * checked, and the file is looked at read-only -- it holds /hit_indices of extent M x k and none of the datasets to add -- before it
 * is opened for writing: a file this call cannot finish is left as it was. */
int sa_host_write_search_values(const char *path, const struct sa_host_store *db, const struct sa_host_store *queries, int32_t k,
				const int32_t *value, int32_t kind, int32_t source, int32_t rule_or_denom, const int32_t *denominators,
				const int32_t *vrect);
/* --query --hits-min: the one writer of a threshold search.  A NEW file at `path` with /sequences (N), /query_sequences (M), the hits
 * of every query as the CSR of sa_hip_search_above -- /hitlist_offsets (M + 1 I64LE), /hitlist_indices and /hitlist_scores (E =
 * offsets[M] I32LE each; extent 0 when E = 0; row q's indices ascending, the scores raw) -- and /hitlist_min (1 I32LE: the
 * threshold).  kind 0: raw scores, `value`, `source`, `rule_or_denom`, `denominators` and `vrect` are not looked at; kind 1 / 2, numbered
 * and checked as sa_host_write_search_values has them: also /hitlist_values (E I32LE, parts per million), /hit_quantity, /hit_scale and,
 * kind 1, /database_denominators (N) and /query_denominators (M) from `denominators` (N + M), with `vrect` (or NULL) /query_values
 * (M x N).  With `rect` (or NULL) /query_scores (M x N).  With `alignments` != 0 also /hitlist_alignment_records (E x 8),
 * /hitlist_cigar_offsets (E + 1 I64LE) and /hitlist_cigars (`runs` U32LE) in the format of the neighbour datasets (a = the query, b =
 * its hit); `records` may be NULL when E = 0.  No /similarity_matrix.  offsets[0] != 0, decreasing offsets, an index outside [0, N)
 * or a row not in ascending index give an error before anything is opened; a file that fails later is removed. */
int sa_host_write_search_list(const char *path, const struct sa_host_store *db, const struct sa_host_store *queries, const int64_t *offsets,
			      const int32_t *index, const int32_t *score, int32_t min_value, const int32_t *value, int32_t kind, int32_t source,
			      int32_t rule_or_denom, const int32_t *denominators, const int32_t *rect, const int32_t *vrect, int alignments,
			      const struct sa_aln *records, const uint32_t *cigar, int64_t runs);
/* --query --strands both: the strands of a folded search (sa_hip_search_strands / sa_hip_search_above_strands), added to the finished
 * file of sa_host_write_search (k >= 1, count < 0: /hit_strands, M x k U8, from hit_strands) or of sa_host_write_search_list (k = 0,
 * count = E >= 0: /hitlist_strands, E U8, from list_strands; extent 0 when E = 0); with rect_strands /query_strands (M x N U8), with
 * reverse_denominators /query_reverse_denominators (M I32LE).  0 = forward, 1 = reverse; another byte, a file without the hits of
 * that shape or one that holds a dataset already give an error and leave the file as it was. */
int sa_host_write_search_strands(const char *path, const struct sa_host_store *db, const struct sa_host_store *queries, int32_t k,
				 const uint8_t *hit_strands, int64_t count, const uint8_t *list_strands, const uint8_t *rect_strands,
				 const int32_t *reverse_denominators);
/* --query --fit: where the query of every hit sits in its database sequence (sa_hip_search_fit), added to the finished file of
 * sa_host_write_search: /hit_db_begin and /hit_db_end (M x k I32LE, the half-open span of database sequence index[q][t]) and
 * /search_ends (1 I32LE: 1 = the database's ends are free).  A span outside its database sequence, a file without /hit_indices of
 * M x k or one that holds a dataset already give an error and leave the file as it was. */
int sa_host_write_search_fit(const char *path, const struct sa_host_store *db, const struct sa_host_store *queries, int32_t k,
			     const int32_t *index, const int32_t *db_begin, const int32_t *db_end);
/* --min-score: /edge_offsets (N + 1 I64LE), /edge_indices and /edge_scores (E = offsets[N] I32LE each; extent 0 when E = 0),
 * the CSR arrays of sa_hip_edges / sa_zjob_edges.  `create` as in sa_host_write_neighbors: 0 adds the three datasets to the
 * finished file at `path`, 1 writes a new file with /sequences and the three (--edges-only).  offsets[0] != 0, decreasing
 * offsets or an index outside [0, N) give an error, and no file when `create` is set. */
int sa_host_write_edges(const char *path, const struct sa_host_store *s, const int64_t *offsets, const int32_t *index, const int32_t *score,
			int create);
/* --linkage / --clusters: /linkage_pairs ((N - 1) x 2 I32LE) and /linkage_scores (N - 1 I32LE), the tree of sa_hip_linkage /
 * sa_zjob_linkage; with `labels` (or NULL) also /cluster_labels (N I32LE).  `create` as in sa_host_write_edges: 1 writes a new
 * file with /sequences and these (--linkage-only).  An index outside [0, N), lo >= hi or a label above its own index give an
 * error, and no file when `create` is set. */
int sa_host_write_linkage(const char *path, const struct sa_host_store *s, const int32_t *pairs, const int32_t *score, const int32_t *labels,
			  int create);
/* --min-quantile / --clusters-quantile / --quantiles: /score_quantiles (m F64LE, the fractions as given), /score_quantile_values
 * (m I32LE) and /score_quantile_below (m I64LE), what sa_hip_select / sa_zjob_select returned for the ranks of the fractions; with
 * `edge_min` (or NULL) also /edge_min_score (1 I32LE), with `cluster_min` (or NULL) also /cluster_min_score (1 I32LE).  `create` as
 * in sa_host_write_edges.  An m outside 1-16, a fraction outside [0, 1] or a count outside [0, P) give an error, and no file when
 * `create` is set. */
int sa_host_write_quantiles(const char *path, const struct sa_host_store *s, const double *fractions, const int32_t *values,
			    const int64_t *below, int32_t m, const int32_t *edge_min, const int32_t *cluster_min, int create);
/* --normalize: /normalization_denominators (N I32LE, d[k] of include/seqalign_hip.h: struct sa_norm), /normalization_rule
 * (2 I32LE: source, rule) and /normalization_scale (1 I32LE: SA_NORM_SCALE), added to the finished file at `path`, whose other
 * datasets stay as they are.  A source or rule outside its enum gives an error before anything is opened. */
int sa_host_write_normalization(const char *path, const struct sa_host_store *s, const int32_t *denominators, int32_t source, int32_t rule);
/* --identity: /identity_rule (1 I32LE: the denominator, SA_PID_* of include/seqalign_hip.h) and /identity_scale (1 I32LE:
 * SA_NORM_SCALE), added to the finished file at `path`, whose other datasets stay as they are.  0 on success. */
int sa_host_write_identity(const char *path, int32_t denom);
/* --linkage-method: /linkage_method (1 I32LE: 0 single, SA_AGGLO_COMPLETE, SA_AGGLO_AVERAGE of include/seqalign_hip.h), added to
 * the finished file at `path`, whose other datasets stay as they are.  0 on success. */
int sa_host_write_linkage_method(const char *path, int32_t method);

#ifdef __cplusplus
}
#endif
#endif
