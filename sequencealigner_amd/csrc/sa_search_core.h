/* sa_search_core.h -- the host-compilable part of the search (sa_search.hip): where the rows of a query batch sit in the
 * bounded packed range, how a row of the rectangle is cut into segments, and the part + merge selection of the hits done
 * serially.  tests/host_c/search_core_test.cpp runs it under ASan / UBSan against std::partial_sort.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_hits): the candidates of query q are ALL database sequences d in [0, N) with
 * rect[q * N + d]; order: score DESCENDING, then d ASCENDING -- the key of sa_neighbors_core.h, which is unique per
 * candidate, so neither the cut into segments nor the order in which partial lists are merged can change a result.
 *
 * Row split: one wave scans one (row, segment).  With few queries one wave per row would leave the device idle, so every
 * row is cut into S segments such that nq * S waves are about SA_HITS_WAVES.  The merge of a row inserts S * k keys with one
 * wave: S is held to N / max(4 k, SA_HITS_SEG_MIN), so that the merge handles at most a quarter of what the row holds, and to
 * SA_HITS_SEG_MAX; S = 1 when the rows alone fill the device (SA_HITS_ROWS_FILL).  S depends on (N, nq, k) only -- never on the device -- so the
 * scratch size is known without one. */
#ifndef SA_SEARCH_CORE_H
#define SA_SEARCH_CORE_H

#include <stdint.h>

#include "sa_neighbors_core.h"

#define SA_HITS_WAVES 8192  /* waves that fill the device: 256 CUs x 4 SIMDs x 8 (the kernel needs < 64 VGPRs) */
#define SA_HITS_ROWS_FILL 2048 /* rows that fill the device by themselves: two waves for each of 256 x 4 SIMDs */
#define SA_HITS_SEG_MIN 16   /* candidates a segment keeps at least (or 4 k, if that is more) */
#define SA_HITS_SEG_MAX 1024 /* segments of a row at most */

/* first packed index of column j: j (j - 1) / 2 */
static inline SA_NB_HD int64_t sa_search_tri(int64_t j) { return j * (j - 1) / 2; }
/* where row q of a batch that begins at query q0 starts in the bounded range [tri(N + q0), ...), in elements */
static inline SA_NB_HD int64_t sa_search_row_at(int64_t n_db, int64_t q0, int64_t q) { return sa_search_tri(n_db + q) - sa_search_tri(n_db + q0); }
/* elements of the range of queries [q0, q0 + nq) */
static inline SA_NB_HD int64_t sa_search_range_elems(int64_t n_db, int64_t q0, int64_t nq) { return sa_search_row_at(n_db, q0, q0 + nq); }

/* segments per row */
static inline SA_NB_HD int32_t sa_hits_segments(int32_t n_db, int32_t nq, int32_t k)
{
	if (nq >= SA_HITS_ROWS_FILL)
		return 1;
	const int64_t seg_min = 4 * (int64_t)k > SA_HITS_SEG_MIN ? 4 * (int64_t)k : SA_HITS_SEG_MIN;
	int64_t s = (SA_HITS_WAVES + (int64_t)nq - 1) / nq;
	if (s > n_db / seg_min)
		s = n_db / seg_min;
	if (s > SA_HITS_SEG_MAX)
		s = SA_HITS_SEG_MAX;
	return (int32_t)(s < 1 ? 1 : s);
}
/* segment s of S covers [sa_hits_seg_begin(n, S, s), sa_hits_seg_begin(n, S, s + 1)): [0, n) once, also for S > n */
static inline SA_NB_HD int32_t sa_hits_seg_begin(int32_t n_db, int32_t S, int32_t s) { return (int32_t)((int64_t)n_db * s / S); }

/* One row, serially, as the two kernels do it: S partial lists of k keys (SA_NB_EMPTY where a segment has fewer than k
 * candidates) into part[S * k], then the merge of those keys.  1 <= k <= min(n_db, 64); S >= 1 (the caller checks). */
static inline void sa_hits_select_row(const int32_t *row, int32_t n_db, int32_t k, int32_t S, uint64_t *part, int32_t *index, int32_t *score)
{
	for (int32_t s = 0; s < S; s++) {
		uint64_t *list = part + (int64_t)s * k;
		for (int32_t t = 0; t < k; t++)
			list[t] = SA_NB_EMPTY;
		for (int32_t d = sa_hits_seg_begin(n_db, S, s); d < sa_hits_seg_begin(n_db, S, s + 1); d++)
			sa_nb_insert(list, k, sa_nb_key(row[d], d));
	}
	uint64_t list[64];
	for (int32_t t = 0; t < k; t++)
		list[t] = SA_NB_EMPTY;
	for (int64_t t = 0; t < (int64_t)S * k; t++)
		sa_nb_insert(list, k, part[t]); /* (an empty entry is below every list and never enters) */
	for (int32_t t = 0; t < k; t++) {
		index[t] = sa_nb_key_index(list[t]);
		score[t] = sa_nb_key_score(list[t]);
	}
}

#endif /* SA_SEARCH_CORE_H */
