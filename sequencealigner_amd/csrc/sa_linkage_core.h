/* sa_linkage_core.h -- the contract of the single-linkage tree (sa_linkage.hip), in a form the host compiles as well:
 * tests/host_c/linkage_test.cpp runs it under ASan / UBSan against a brute-force Kruskal and a double loop.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_linkage).  Pair i < j sits at packed index p = j (j - 1) / 2 + i.  Pair e comes
 * BEFORE pair f iff score(e) > score(f), or the scores are equal and p(e) < p(f): a strict total order, under which the maximum
 * spanning tree of the complete graph is unique.  The tree is its N - 1 pairs in that order (best first): the order in which
 * Kruskal's algorithm, and so single linkage, joins clusters.  Cutting it at T leaves the connected components of the graph
 * score >= T.
 *
 * What the kernels and the host share: the order predicate, the packed index and its inverse, and the ROOT RULE of a Boruvka
 * round.  Every component C picks the best pair that leaves it and takes the component D at that pair's other end as its
 * parent.  Under a strict total order the only cycles of these hooks are mutual ones (C picks D and D picks C), and then both
 * picked the same pair: the smaller id of the two stays a root, the other records the pair, once.  sa_lk_parent is that rule.
 *
 * Host only: the serial tree (Prim, O(N^2)), the labels at a threshold and the merge table. */
#ifndef SA_LINKAGE_CORE_H
#define SA_LINKAGE_CORE_H

#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>

#include "sa_neighbors_core.h" /* SA_NB_HD, sa_nb_packed_at */

/* the order: does the pair (score e, packed index pe) come before (score f, packed index pf)? */
static inline SA_NB_HD bool sa_lk_before(int32_t e, int64_t pe, int32_t f, int64_t pf) { return e > f || (e == f && pe < pf); }

/* pair (r, c), r != c, in the packed triangle */
static inline SA_NB_HD int64_t sa_lk_packed_at(int64_t r, int64_t c) { return sa_nb_packed_at(r, c); }

/* ... and back: p = hi (hi - 1) / 2 + lo with lo < hi.  The square root lands within one of hi; the two loops (at most a few
 * steps each, whatever p) make it exact.  p >= 0. */
static inline SA_NB_HD void sa_lk_unpack(int64_t p, int64_t *lo, int64_t *hi)
{
	int64_t j = (int64_t)((1.0 + __builtin_sqrt(1.0 + 8.0 * (double)p)) * 0.5);
	if (j < 1)
		j = 1;
	for (int step = 0; step < 4 && j * (j - 1) / 2 > p; step++)
		j--;
	for (int step = 0; step < 4 && (j + 1) * j / 2 <= p; step++)
		j++;
	*hi = j;
	*lo = p - j * (j - 1) / 2;
}

/* the root rule: component c picked the pair pc, which ends in component d; pd is the pair d picked (any value that is no
 * packed index when d picked none).  Returns c's parent; c records its pair iff the parent is not c itself. */
static inline SA_NB_HD int32_t sa_lk_parent(int32_t c, int32_t d, int64_t pc, int64_t pd)
{
	if (pd == pc) /* mutual: both picked this pair */
		return c < d ? c : d;
	return d;
}

/* ---- host only ------------------------------------------------------------------------------------------------------------ */

struct sa_lk_edge {
	int32_t score, lo, hi;
	int64_t p;
};

static inline int sa_lk_edge_cmp(const void *a, const void *b)
{
	const struct sa_lk_edge *e = (const struct sa_lk_edge *)a, *f = (const struct sa_lk_edge *)b;
	if (sa_lk_before(e->score, e->p, f->score, f->p))
		return -1;
	return sa_lk_before(f->score, f->p, e->score, e->p) ? 1 : 0;
}

/* the tree of a packed matrix, serially: Prim from vertex 0, then sorted.  pairs: 2 (num - 1), score: num - 1.
 * Returns 0, or 1 when the host has no memory for 4 num words of work space. */
static inline int sa_lk_tree_serial(const int32_t *packed, int32_t num, int32_t *pairs, int32_t *score)
{
	if (num < 2)
		return 0;
	const size_t n = (size_t)num;
	int32_t *best = (int32_t *)malloc(n * sizeof(int32_t)); /* best pair from v into the tree: its score ... */
	int64_t *bestp = (int64_t *)malloc(n * sizeof(int64_t)); /* ... and packed index */
	bool *in = (bool *)calloc(n, sizeof(bool));
	struct sa_lk_edge *edges = (struct sa_lk_edge *)malloc((n - 1) * sizeof(struct sa_lk_edge));
	int rc = 1;
	if (best && bestp && in && edges) {
		int32_t last = 0;
		in[0] = true;
		for (int32_t v = 1; v < num; v++)
			bestp[v] = -1;
		for (int32_t t = 0; t + 1 < num; t++) {
			int32_t pick = -1;
			for (int32_t v = 0; v < num; v++) {
				if (in[v])
					continue;
				const int64_t p = sa_lk_packed_at(v, last);
				if (bestp[v] < 0 || sa_lk_before(packed[p], p, best[v], bestp[v])) {
					best[v] = packed[p];
					bestp[v] = p;
				}
				if (pick < 0 || sa_lk_before(best[v], bestp[v], best[pick], bestp[pick]))
					pick = v;
			}
			int64_t lo, hi;
			sa_lk_unpack(bestp[pick], &lo, &hi);
			edges[t].score = best[pick];
			edges[t].p = bestp[pick];
			edges[t].lo = (int32_t)lo;
			edges[t].hi = (int32_t)hi;
			in[pick] = true;
			last = pick;
		}
		qsort(edges, n - 1, sizeof(struct sa_lk_edge), sa_lk_edge_cmp);
		for (size_t t = 0; t + 1 < n; t++) {
			pairs[2 * t] = edges[t].lo;
			pairs[2 * t + 1] = edges[t].hi;
			score[t] = edges[t].score;
		}
		rc = 0;
	}
	free(best);
	free(bestp);
	free(in);
	free(edges);
	return rc;
}

/* union-find over 0 .. num - 1 in which the root of a set is its SMALLEST member */
static inline int32_t sa_lk_find(int32_t *up, int32_t v)
{
	int32_t root = v;
	while (up[root] != root)
		root = up[root];
	while (up[v] != root) {
		const int32_t next = up[v];
		up[v] = root;
		v = next;
	}
	return root;
}

enum { SA_LK_OK = 0, SA_LK_RANGE = -1, SA_LK_LO_HI = -2, SA_LK_CYCLE = -3, SA_LK_ORDER = -4, SA_LK_MEMORY = -5 };

/* is it a tree?  every index in 0 .. num - 1, lo < hi, no cycle; with `score`, the pairs in the contract's order.
 * `up`: num words of work space. */
static inline int sa_lk_check(const int32_t *pairs, const int32_t *score, int32_t num, int32_t *up)
{
	for (int32_t v = 0; v < num; v++)
		up[v] = v;
	for (int32_t t = 0; t + 1 < num; t++) {
		const int32_t lo = pairs[2 * t], hi = pairs[2 * t + 1];
		if (lo < 0 || hi < 0 || lo >= num || hi >= num)
			return SA_LK_RANGE;
		if (lo >= hi)
			return SA_LK_LO_HI;
		const int32_t a = sa_lk_find(up, lo), b = sa_lk_find(up, hi);
		if (a == b)
			return SA_LK_CYCLE;
		up[a > b ? a : b] = a > b ? b : a;
		if (score && t > 0 &&
		    !sa_lk_before(score[t - 1], sa_lk_packed_at(pairs[2 * t - 2], pairs[2 * t - 1]), score[t], sa_lk_packed_at(lo, hi)))
			return SA_LK_ORDER;
	}
	return SA_LK_OK;
}

/* labels[r] = the smallest index in r's component of the graph score >= min_score.  Returns the number of clusters, or one
 * of the negative codes above with nothing written. */
static inline int32_t sa_lk_labels(const int32_t *pairs, const int32_t *score, int32_t num, int32_t min_score, int32_t *labels)
{
	int32_t *up = (int32_t *)malloc((size_t)num * sizeof(int32_t));
	if (!up)
		return SA_LK_MEMORY;
	const int bad = sa_lk_check(pairs, score, num, up);
	if (bad) {
		free(up);
		return bad;
	}
	for (int32_t v = 0; v < num; v++)
		up[v] = v;
	int32_t clusters = num;
	for (int32_t t = 0; t + 1 < num && score[t] >= min_score; t++) { /* (in order: the first one below ends it) */
		const int32_t a = sa_lk_find(up, pairs[2 * t]), b = sa_lk_find(up, pairs[2 * t + 1]);
		up[a > b ? a : b] = a > b ? b : a;
		clusters--;
	}
	for (int32_t v = 0; v < num; v++)
		labels[v] = sa_lk_find(up, v);
	free(up);
	return clusters;
}

/* the merge table in the convention of scipy.cluster.hierarchy: merge t joins clusters left[t] < right[t]; ids below num are
 * sequences, id num + u is the cluster made by merge u; size[t] = sequences in the new cluster.  0, or a negative code with
 * nothing written. */
static inline int sa_lk_merges(const int32_t *pairs, int32_t num, int32_t *left, int32_t *right, int32_t *size)
{
	int32_t *up = (int32_t *)malloc(3 * (size_t)num * sizeof(int32_t));
	if (!up)
		return SA_LK_MEMORY;
	const int bad = sa_lk_check(pairs, NULL, num, up);
	if (bad) {
		free(up);
		return bad;
	}
	int32_t *id = up + num, *members = id + num; /* of the set whose root is v */
	for (int32_t v = 0; v < num; v++) {
		up[v] = v;
		id[v] = v;
		members[v] = 1;
	}
	for (int32_t t = 0; t + 1 < num; t++) {
		const int32_t a = sa_lk_find(up, pairs[2 * t]), b = sa_lk_find(up, pairs[2 * t + 1]);
		const int32_t root = a < b ? a : b, other = a < b ? b : a;
		left[t] = id[a] < id[b] ? id[a] : id[b];
		right[t] = id[a] < id[b] ? id[b] : id[a];
		size[t] = members[a] + members[b];
		up[other] = root;
		id[root] = num + t;
		members[root] = size[t];
	}
	free(up);
	return SA_LK_OK;
}

#endif /* SA_LINKAGE_CORE_H */
