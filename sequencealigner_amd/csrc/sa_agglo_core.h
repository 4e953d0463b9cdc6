/* sa_agglo_core.h -- the contract of complete and average linkage (sa_agglo.hip), in a form the host compiles as well:
 * tests/host_c/agglo_test.cpp runs it under ASan / UBSan against a brute-force restatement and replays the device's steps.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_agglomerate).  A cluster is named by its smallest member.  The similarity of two
 * clusters is, COMPLETE: the minimum score over their cross pairs (int32); AVERAGE: the exact rational S / n, S the int64 sum
 * of those scores and n = |A| |B|.  Cluster pair e = (A, B) with names a < b has p(e) = b (b - 1) / 2 + a; e comes BEFORE f iff
 * sim(e) > sim(f), or the similarities are equal and p(e) < p(f).  Two averages are compared by cross-multiplication in 128
 * bits: no floating point anywhere.  Step t merges the first pair among all pairs of active clusters; the union keeps the name
 * a; its similarity to every other cluster C is min(sim(A, C), sim(B, C)), or S(A, C) + S(B, C) with size |A| + |B|.
 *
 * What the kernels and the host share: the order predicate, the two combine rules, the floor division of the reported average,
 * the position in the square working matrix, and the CACHE RULE.  Row c of the working matrix caches best[c], the partner that
 * comes first among the active clusters other than c.  After A and B have merged into A, the only entry of row c that changed
 * is (c, a), and (c, b) is gone:
 *   best[c] was neither a nor b: the new entry is compared with the cached one;
 *   best[c] was a or b: every other entry came AFTER the cached key already, so when the new entry does not come after that
 *                       key it is the first of the row -- kept without a scan; otherwise the row is scanned again.
 * Comparisons inside one row leave the common factor |C| out of n: n is the partner's size there, the product in sa_ag_pick.
 *
 * Host only: the serial greedy tree (O(N^3), the definition), and the labels at a threshold. */
#ifndef SA_AGGLO_CORE_H
#define SA_AGGLO_CORE_H

#include "sa_linkage_core.h" /* sa_lk_before, sa_lk_packed_at, sa_lk_check, sa_lk_find, SA_NB_HD */

#define SA_AGGLO_SINGLE 0 /* reserved: sa_ctx_linkage */
#define SA_AGGLO_COMPLETE 1
#define SA_AGGLO_AVERAGE 2
#define SA_AGGLO_AVERAGE_MAX_NUM 131072 /* |S| <= 2^31 N^2 / 4 <= 2^63 */
#define SA_AGGLO_COMPLETE_MAX_NUM (1 << 30) /* (the working matrix passes 2^62 bytes beyond it) */

/* -1, 0, 1: S1 / n1 below, equal to, above S2 / n2; n1, n2 > 0.  |S| < 2^63 and n < 2^63: the products fit 128 bits. */
static inline SA_NB_HD int sa_ag_cmp_avg(int64_t s1, int64_t n1, int64_t s2, int64_t n2)
{
	const __int128 l = (__int128)s1 * n2, r = (__int128)s2 * n1;
	return l > r ? 1 : l < r ? -1 : 0;
}

/* floor(s / n), n > 0, rounded towards minus infinity (Python's //, as sa_norm_value) */
static inline SA_NB_HD int64_t sa_ag_floor_div(int64_t s, int64_t n)
{
	int64_t q = s / n;
	if (s % n != 0 && s < 0)
		q--;
	return q;
}

/* position (r, c) of the square working matrix */
static inline SA_NB_HD int64_t sa_ag_at(int64_t r, int64_t c, int64_t num) { return r * num + c; }

/* a method's similarity type and rules; n is ignored by complete linkage */
template <int METHOD> struct sa_ag_rule;

template <> struct sa_ag_rule<SA_AGGLO_COMPLETE> {
	typedef int32_t T;
	static inline SA_NB_HD int cmp(T s1, int64_t, T s2, int64_t) { return s1 > s2 ? 1 : s1 < s2 ? -1 : 0; }
	static inline SA_NB_HD T combine(T x, T y) { return x < y ? x : y; }
	static inline SA_NB_HD int32_t score(T s, int64_t) { return s; }
};

template <> struct sa_ag_rule<SA_AGGLO_AVERAGE> {
	typedef int64_t T;
	static inline SA_NB_HD int cmp(T s1, int64_t n1, T s2, int64_t n2) { return sa_ag_cmp_avg(s1, n1, s2, n2); }
	static inline SA_NB_HD T combine(T x, T y) { return x + y; }
	static inline SA_NB_HD int32_t score(T s, int64_t n) { return (int32_t)sa_ag_floor_div(s, n); } /* (an average of int32 values) */
};

/* the order: does (s1 / n1, packed index p1) come before (s2 / n2, p2)? */
template <int METHOD>
static inline SA_NB_HD bool sa_ag_before(typename sa_ag_rule<METHOD>::T s1, int64_t n1, int64_t p1, typename sa_ag_rule<METHOD>::T s2,
					 int64_t n2, int64_t p2)
{
	const int c = sa_ag_rule<METHOD>::cmp(s1, n1, s2, n2);
	return c > 0 || (c == 0 && p1 < p2);
}

/* the size cluster o had BEFORE the merge of b into a; size[] is read after it (size[a] grown by size[b], size[b] left) */
static inline SA_NB_HD int32_t sa_ag_size_before(const int32_t *size, int32_t o, int32_t a, int32_t b)
{
	return o == a ? size[a] - size[b] : size[o];
}

enum { SA_AG_KEEP = 0, SA_AG_TAKE = 1, SA_AG_RESCAN = 2 };

/* the cache rule of row c after b has merged into a (c is neither): `old` = best[c] with the similarity (old_s, old_n) it had
 * before the merge, (new_s, new_n) = the new entry (c, a).  KEEP: best[c] stays; TAKE: best[c] = a; RESCAN: scan the row. */
template <int METHOD>
static inline SA_NB_HD int sa_ag_cache(int32_t c, int32_t a, int32_t b, int32_t old, typename sa_ag_rule<METHOD>::T old_s, int64_t old_n,
				       typename sa_ag_rule<METHOD>::T new_s, int64_t new_n)
{
	const int64_t p_old = sa_lk_packed_at(c, old), p_new = sa_lk_packed_at(c, a);
	if (old != a && old != b)
		return sa_ag_before<METHOD>(new_s, new_n, p_new, old_s, old_n, p_old) ? SA_AG_TAKE : SA_AG_KEEP;
	return sa_ag_before<METHOD>(old_s, old_n, p_old, new_s, new_n, p_new) ? SA_AG_RESCAN : SA_AG_TAKE;
}

/* ---- host only ------------------------------------------------------------------------------------------------------------ */

enum { SA_AG_NOT_DESCENDING = -6 }; /* beside the SA_LK_* codes */

/* the tree of a packed matrix by the definition: a full working matrix, every step looks at every pair of active clusters.
 * pairs: 2 (num - 1), score: num - 1.  Returns 0, or 1 when the host has no memory. */
template <int METHOD> static inline int sa_ag_tree_serial(const int32_t *packed, int32_t num, int32_t *pairs, int32_t *score)
{
	typedef typename sa_ag_rule<METHOD>::T T;
	if (num < 2)
		return 0;
	const size_t n = (size_t)num;
	T *w = (T *)malloc(n * n * sizeof(T));
	int32_t *size = (int32_t *)malloc(n * sizeof(int32_t));
	int rc = 1;
	if (w && size) {
		for (int32_t r = 0; r < num; r++) {
			size[r] = 1;
			for (int32_t c = 0; c < num; c++)
				w[sa_ag_at(r, c, num)] = r == c ? 0 : packed[sa_lk_packed_at(r, c)];
		}
		for (int32_t t = 0; t + 1 < num; t++) {
			int32_t a = -1, b = -1;
			for (int32_t j = 1; j < num; j++) /* (size 0: merged away) */
				for (int32_t i = 0; size[j] && i < j; i++) {
					if (!size[i])
						continue;
					if (a < 0 || sa_ag_before<METHOD>(w[sa_ag_at(i, j, num)], (int64_t)size[i] * size[j], sa_lk_packed_at(i, j),
									  w[sa_ag_at(a, b, num)], (int64_t)size[a] * size[b], sa_lk_packed_at(a, b))) {
						a = i;
						b = j;
					}
				}
			pairs[2 * t] = a;
			pairs[2 * t + 1] = b;
			score[t] = sa_ag_rule<METHOD>::score(w[sa_ag_at(a, b, num)], (int64_t)size[a] * size[b]);
			for (int32_t c = 0; c < num; c++)
				if (size[c] && c != a && c != b)
					w[sa_ag_at(a, c, num)] = w[sa_ag_at(c, a, num)] =
						sa_ag_rule<METHOD>::combine(w[sa_ag_at(a, c, num)], w[sa_ag_at(b, c, num)]);
			size[a] += size[b];
			size[b] = 0;
		}
		rc = 0;
	}
	free(w);
	free(size);
	return rc;
}

/* labels[r] = the smallest index in r's cluster after the merges t with score[t] >= min_score -- a prefix, since the scores do
 * not increase.  Returns the number of clusters, or a negative code with nothing written: one of sa_lk_check's for pairs that
 * are no tree, SA_AG_NOT_DESCENDING for scores that increase. */
static inline int32_t sa_ag_labels(const int32_t *pairs, const int32_t *score, int32_t num, int32_t min_score, int32_t *labels)
{
	int32_t *up = (int32_t *)malloc((size_t)num * sizeof(int32_t));
	if (!up)
		return SA_LK_MEMORY;
	int bad = sa_lk_check(pairs, NULL, num, up);
	for (int32_t t = 1; !bad && t + 1 < num; t++)
		if (score[t] > score[t - 1])
			bad = SA_AG_NOT_DESCENDING;
	if (bad) {
		free(up);
		return bad;
	}
	for (int32_t v = 0; v < num; v++)
		up[v] = v;
	int32_t clusters = num;
	for (int32_t t = 0; t + 1 < num && score[t] >= min_score; t++) {
		const int32_t a = sa_lk_find(up, pairs[2 * t]), b = sa_lk_find(up, pairs[2 * t + 1]);
		up[a > b ? a : b] = a > b ? b : a;
		clusters--;
	}
	for (int32_t v = 0; v < num; v++)
		labels[v] = sa_lk_find(up, v);
	free(up);
	return clusters;
}

#endif /* SA_AGGLO_CORE_H */
