/* sa_select_core.h -- the contract of the order statistics of the score distribution (sa_select.hip), in a form the host
 * compiles as well: tests/host_c/select_test.cpp runs it under ASan / UBSan against std::sort.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_select): s_0 <= s_1 <= ... <= s_{P-1} are the P = N (N - 1) / 2 entries of the packed
 * triangle in ascending order; for a rank k in [0, P), value = s_k and below = the number of entries < s_k.
 *
 * A radix select, most significant byte first.  key = score with the sign bit flipped: unsigned order of the keys = signed order
 * of the scores.  A rank carries the key PREFIX found so far (the upper 8 * round bits, the rest zero), the rank REMAINING among
 * the entries that share the prefix, and BELOW = the entries whose key is smaller than every key with that prefix.  A round
 *   counts   for every distinct prefix (a GROUP: at most one per rank), the entries that share it, by their next byte: a table
 *            of 256 64-bit counts per group.  Entries that share no group's prefix are dropped;
 *   narrows  per rank: walks the 256 bins of its group upwards until the running sum exceeds the remaining rank; that bin is
 *            the next byte of s_k, the sum before it leaves the remaining rank and joins below;
 *   regroups the distinct new prefixes, in the order of the first rank that holds each, are the groups of the next round.
 * After four rounds the prefix is the key of s_k.  Counts are sums of integers: no result depends on the order in which
 * entries, waves or workgroups are counted.  The kernels call the functions below; sa_sel_count is their count with a loop. */
#ifndef SA_SELECT_CORE_H
#define SA_SELECT_CORE_H

#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "sa_neighbors_core.h" /* SA_NB_HD */

#define SA_SEL_MAX 16    /* = SA_HIP_SELECT_MAX */
#define SA_SEL_ROUNDS 4
#define SA_SEL_BINS 256

/* the key: order-preserving, its own inverse */
static inline SA_NB_HD uint32_t sa_sel_key(int32_t score) { return (uint32_t)score ^ 0x80000000u; }
static inline SA_NB_HD int32_t sa_sel_score(uint32_t key) { return (int32_t)(key ^ 0x80000000u); }

/* round 0 .. 3 looks at bits shift .. shift + 7 */
static inline SA_NB_HD int sa_sel_shift(int round) { return 24 - 8 * round; }
static inline SA_NB_HD uint32_t sa_sel_byte(uint32_t key, int round) { return (key >> sa_sel_shift(round)) & 255u; }
/* the 8 * round upper bits of a key, which a group's prefix fixes (round 0: none, always 0; never above 2^24 - 1) */
static inline SA_NB_HD uint32_t sa_sel_upper(uint32_t key, int round) { return round == 0 ? 0u : key >> (32 - 8 * round); }
/* does `key` share them with `prefix`? */
static inline SA_NB_HD bool sa_sel_shares(uint32_t key, uint32_t prefix, int round)
{
	return sa_sel_upper(key, round) == sa_sel_upper(prefix, round);
}
#define SA_SEL_NO_UPPER 0xFFFFFFFFu /* what sa_sel_upper never returns */

/* what d_scratch holds: this, then the table uint64[m][256] */
struct sa_sel_state {
	int64_t remain[SA_SEL_MAX];        /* per rank: the rank among the entries that share its prefix */
	int64_t below[SA_SEL_MAX];         /* per rank: entries with a smaller key than any of those */
	uint32_t prefix[SA_SEL_MAX];       /* per rank */
	int32_t group_of[SA_SEL_MAX];      /* per rank: its group in this round */
	uint32_t group_prefix[SA_SEL_MAX]; /* per group */
	int32_t groups, pad;
};

static inline SA_NB_HD size_t sa_sel_table_offset(void) { return sizeof(struct sa_sel_state); }
/* 0 for an m outside [1, SA_SEL_MAX] */
static inline SA_NB_HD size_t sa_sel_scratch_bytes(int32_t m)
{
	return m < 1 || m > SA_SEL_MAX ? 0 : sa_sel_table_offset() + (size_t)m * SA_SEL_BINS * sizeof(uint64_t);
}

/* fraction -> rank: min(pairs - 1, floor(q * pairs)) with the plain double product; -1 for what is no fraction or no matrix */
static inline int64_t sa_sel_rank(int64_t pairs, double q)
{
	if (pairs < 1 || !(q >= 0.0 && q <= 1.0)) /* (a NaN fails both comparisons) */
		return -1;
	const double at = floor(q * (double)pairs);
	if (at >= (double)(pairs - 1)) /* (also keeps the conversion below in range) */
		return pairs - 1;
	const int64_t rank = (int64_t)at;
	return rank < pairs - 1 ? rank : pairs - 1;
}

/* rank t before round 0: one group, the empty prefix */
static inline SA_NB_HD void sa_sel_start(struct sa_sel_state *st, int t, int64_t rank)
{
	st->remain[t] = rank;
	st->below[t] = 0;
	st->prefix[t] = 0;
	st->group_of[t] = 0;
	if (t == 0) {
		st->group_prefix[0] = 0;
		st->groups = 1;
		st->pad = 0;
	}
}

/* rank t after the count of `round`: table = uint64[groups][256] */
static inline SA_NB_HD void sa_sel_narrow(struct sa_sel_state *st, const uint64_t *table, int t, int round)
{
	const uint64_t *bins = table + (size_t)st->group_of[t] * SA_SEL_BINS;
	const int64_t remain = st->remain[t];
	int64_t before = 0;
	int bin = 0;
	for (; bin < SA_SEL_BINS - 1; bin++) { /* (a rank inside [0, P) ends before the last bin or in it) */
		const int64_t n = (int64_t)bins[bin];
		if (before + n > remain)
			break;
		before += n;
	}
	st->prefix[t] |= (uint32_t)bin << sa_sel_shift(round);
	st->remain[t] = remain - before;
	st->below[t] += before;
}

/* the groups of the next round from the prefixes of the m ranks: distinct values in the order of first appearance, so never
 * more than m */
static inline SA_NB_HD void sa_sel_regroup(struct sa_sel_state *st, int32_t m)
{
	int32_t groups = 0;
	for (int32_t t = 0; t < m; t++) {
		int32_t g = 0;
		while (g < groups && st->group_prefix[g] != st->prefix[t])
			g++;
		if (g == groups)
			st->group_prefix[groups++] = st->prefix[t];
		st->group_of[t] = g;
	}
	st->groups = groups;
}

/* which group an entry counts for in `round`, -1 for none (prefixes are distinct: at most one) */
static inline SA_NB_HD int sa_sel_group(uint32_t key, const uint32_t *group_prefix, int32_t groups, int round)
{
	int found = -1;
	for (int32_t g = 0; g < groups; g++)
		if (sa_sel_shares(key, group_prefix[g], round))
			found = g;
	return found;
}

/* the count of a round, serially: table must be zero */
static inline void sa_sel_count(const int32_t *packed, int64_t pairs, const struct sa_sel_state *st, int round, uint64_t *table)
{
	for (int64_t p = 0; p < pairs; p++) {
		const uint32_t key = sa_sel_key(packed[p]);
		const int g = sa_sel_group(key, st->group_prefix, st->groups, round);
		if (g >= 0)
			table[(size_t)g * SA_SEL_BINS + sa_sel_byte(key, round)]++;
	}
}

/* the whole select, serially: st and table (m * 256) are the caller's; ranks inside [0, pairs), 1 <= m <= SA_SEL_MAX.
 * max_groups (may be NULL): the most groups any round had. */
static inline void sa_sel_serial(const int32_t *packed, int64_t pairs, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below,
				 struct sa_sel_state *st, uint64_t *table, int32_t *max_groups)
{
	for (int32_t t = 0; t < m; t++)
		sa_sel_start(st, t, ranks[t]);
	if (max_groups)
		*max_groups = 1;
	for (int round = 0; round < SA_SEL_ROUNDS; round++) {
		for (size_t b = 0; b < (size_t)m * SA_SEL_BINS; b++)
			table[b] = 0;
		sa_sel_count(packed, pairs, st, round, table);
		for (int32_t t = 0; t < m; t++)
			sa_sel_narrow(st, table, t, round);
		sa_sel_regroup(st, m);
		if (max_groups && st->groups > *max_groups)
			*max_groups = st->groups;
	}
	for (int32_t t = 0; t < m; t++) {
		value[t] = sa_sel_score(st->prefix[t]);
		below[t] = st->below[t];
	}
}

#endif /* SA_SELECT_CORE_H */
