/* sa_neighbors_core.h -- the ordering contract of the nearest-neighbour selection (sa_neighbors.hip), in a form the host
 * compiles as well: tests/host_c/neighbors_test.cpp runs it under ASan / UBSan against std::partial_sort.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_neighbors): the candidates of sequence r are all c != r with the symmetric matrix
 * entry score(r, c); they are ordered by score DESCENDING, then index c ASCENDING; row r of the result holds the first k.
 *
 * One 64-bit KEY carries that order -- a larger key is a better candidate -- so that a tie can never depend on the order in
 * which candidates arrive:  high word = score with the sign bit flipped (unsigned order = signed order), low word = ~c
 * (a smaller index is the larger word).  c <= INT32_MAX makes the low word of every real key >= 0x80000000: key 0 is below
 * every candidate and marks an empty list entry.
 *
 * The list of a row is k keys in descending order.  A candidate is compared with the k-th entry first; only one that beats
 * it is inserted: its position is the number of entries above it, the entries from there on move down by one.  The kernel
 * keeps the list one entry per lane and does exactly these three steps with a ballot, a population count and a one-lane
 * shift; sa_nb_insert is the same thing with loops. */
#ifndef SA_NEIGHBORS_CORE_H
#define SA_NEIGHBORS_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define SA_NB_HD __host__ __device__
#else
#define SA_NB_HD
#endif

#define SA_NB_EMPTY ((uint64_t)0)

static inline SA_NB_HD uint64_t sa_nb_key(int32_t score, int32_t c)
{
	return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(uint32_t)~(uint32_t)c;
}
static inline SA_NB_HD int32_t sa_nb_key_score(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
static inline SA_NB_HD int32_t sa_nb_key_index(uint64_t key) { return (int32_t)~(uint32_t)key; }

/* where the symmetric entry (r, c), r != c, sits in the packed triangle: pair i < j at j (j - 1) / 2 + i */
static inline SA_NB_HD int64_t sa_nb_packed_at(int64_t r, int64_t c)
{
	const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
	return hi * (hi - 1) / 2 + lo;
}

/* list[0 .. k): descending keys (SA_NB_EMPTY where nothing has arrived yet) */
static inline void sa_nb_insert(uint64_t *list, int32_t k, uint64_t x)
{
	if (!(x > list[k - 1]))
		return;
	int32_t pos = 0;
	for (int32_t t = 0; t < k; t++)
		pos += list[t] > x;
	for (int32_t t = k - 1; t > pos; t--)
		list[t] = list[t - 1];
	list[pos] = x;
}

/* row r of the result, serially: index[0 .. k), score[0 .. k); 1 <= k <= num - 1, k <= 64 (the caller checks) */
static inline void sa_nb_select_row(const int32_t *packed, int32_t num, int32_t r, int32_t k, int32_t *index, int32_t *score)
{
	uint64_t list[64];
	for (int32_t t = 0; t < k; t++)
		list[t] = SA_NB_EMPTY;
	for (int32_t c = 0; c < num; c++)
		if (c != r)
			sa_nb_insert(list, k, sa_nb_key(packed[sa_nb_packed_at(r, c)], c));
	for (int32_t t = 0; t < k; t++) {
		index[t] = sa_nb_key_index(list[t]);
		score[t] = sa_nb_key_score(list[t]);
	}
}

#endif /* SA_NEIGHBORS_CORE_H */
