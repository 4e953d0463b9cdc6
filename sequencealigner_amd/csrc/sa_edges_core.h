/* sa_edges_core.h -- the contract of the score graph (sa_edges.hip), in a form the host compiles as well:
 * tests/host_c/edges_test.cpp runs it under ASan / UBSan against a brute-force double loop.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_edge_offsets): entry (r, c), c != r, is an edge iff score(r, c) >= min_score,
 * score(r, c) the symmetric matrix entry; the diagonal is never a candidate.  The result is the symmetric adjacency as CSR:
 * offsets int64[N + 1] (offsets[0] = 0, offsets[r + 1] - offsets[r] = degree of r), index / score int32[offsets[N]], row r's
 * columns in ASCENDING c.
 *
 * Row r of the symmetric matrix is two pieces of the packed triangle (pair i < j at j (j - 1) / 2 + i): the columns c < r are
 * one contiguous run that starts at sa_edge_left_at(r, 0); a column c > r is the single element sa_edge_right_at(r, c), where
 * consecutive ROWS of one column are contiguous.  The kernels walk the columns in ascending order, so the place of a passing
 * entry is offsets[r] + the number of passing entries before it in the row: nothing depends on which wave arrives first.
 * sa_edge_count_row / sa_edge_fill_row are the same thing with loops. */
#ifndef SA_EDGES_CORE_H
#define SA_EDGES_CORE_H

#include <stdbool.h>
#include <stdint.h>

#include "sa_neighbors_core.h" /* SA_NB_HD, sa_nb_packed_at */

/* the predicate: any int32 threshold is valid */
static inline SA_NB_HD bool sa_edge_pass(int32_t score, int32_t min_score) { return score >= min_score; }

/* the two pieces of row r: c < r (a run along c) and c > r (one element per column) */
static inline SA_NB_HD int64_t sa_edge_left_at(int64_t r, int64_t c) { return r * (r - 1) / 2 + c; }
static inline SA_NB_HD int64_t sa_edge_right_at(int64_t r, int64_t c) { return c * (c - 1) / 2 + r; }

/* degree of row r, serially */
static inline int64_t sa_edge_count_row(const int32_t *packed, int32_t num, int32_t r, int32_t min_score)
{
	int64_t count = 0;
	for (int32_t c = 0; c < r; c++)
		count += sa_edge_pass(packed[sa_edge_left_at(r, c)], min_score);
	for (int32_t c = r + 1; c < num; c++)
		count += sa_edge_pass(packed[sa_edge_right_at(r, c)], min_score);
	return count;
}

/* row r of the result, serially: index / score are the WHOLE arrays, the row starts at `at` (= offsets[r]); returns where
 * the row ends (= offsets[r + 1]) */
static inline int64_t sa_edge_fill_row(const int32_t *packed, int32_t num, int32_t r, int32_t min_score, int64_t at, int32_t *index,
				       int32_t *score)
{
	for (int32_t c = 0; c < num; c++) {
		if (c == r)
			continue;
		const int32_t v = packed[sa_nb_packed_at(r, c)];
		if (sa_edge_pass(v, min_score)) {
			index[at] = c;
			score[at] = v;
			at++;
		}
	}
	return at;
}

/* offsets[0 .. num] from the degrees, serially: the exclusive scan */
static inline void sa_edge_offsets(const int32_t *packed, int32_t num, int32_t min_score, int64_t *offsets)
{
	offsets[0] = 0;
	for (int32_t r = 0; r < num; r++)
		offsets[r + 1] = offsets[r] + sa_edge_count_row(packed, num, r, min_score);
}

#endif /* SA_EDGES_CORE_H */
