/* sa_search_batch_core.h -- the host-compilable part of the one-call search drivers (sa_search_run.h): what a query of a batch
 * costs in device bytes, form by form, and how many queries a batch takes.  tests/host_c/search_batch_test.cpp runs it under
 * ASan / UBSan against the formulas of include/seqalign_hip.h written out.
 *
 * A one-call form keeps on the device, per query of a batch, what grows with the batch: with W = (N + 63) / 64 and
 * s = 2 with both strands, 1 otherwise,
 *   the range row      4 (N + s M)   the longest row of the bounded packed range (N + s M - 1 elements; both halves of a strands
 *                                    batch use the one buffer in turn); none under percent identity, which runs no packed alignment
 *   the rectangles     4 s N raw, 8 s N with a value rectangle beside the raw one
 *   the strand bitmap  8 W
 *   the tail           what the form keeps after the rectangles: the hit lists of a top-k form, the segment counts of a
 *                      threshold form
 * Everything else (partial lists, offsets, segment counts beyond one per query) is inside the quarter of the free memory that the
 * budget leaves alone.  All arithmetic is 64-bit: N = M = 2^31 - 1 overflows nothing. */
#ifndef SA_SEARCH_BATCH_CORE_H
#define SA_SEARCH_BATCH_CORE_H

#include <stdint.h>

struct sa_batch_form {
	bool aligned;  /* a packed alignment runs (not percent identity) */
	bool quantity; /* a value rectangle beside the raw one */
	bool strands;
	int64_t tail;
};

/* the tails.  Top-k: index and score, 8 k, + one partial list, 8 k; by a quantity the value as well, 4 k; with both strands the
 * three arrays whatever the kind, and one byte per hit for its strand.  Nothing without hits. */
static inline int64_t sa_batch_tail_topk(bool hits, bool quantity, bool strands, int32_t k)
{
	return hits ? (int64_t)(strands ? 21 : quantity ? 20 : 16) * k : 0;
}
/* threshold forms: one 64-bit count */
static inline int64_t sa_batch_tail_above(void) { return 8; }

static inline int64_t sa_batch_per_query(int64_t n, int64_t m, struct sa_batch_form f)
{
	const int64_t s = f.strands ? 2 : 1, words = (n + 63) / 64;
	return (f.aligned ? 4 * (n + s * m) : 0) + (f.quantity ? 8 : 4) * s * n + (f.strands ? 8 * words : 0) + f.tail;
}

/* sa_hip_search_fit: a row of the rectangle and of the value rectangle (counted also when the hits are ranked by the score), and
 * with hits index, value, score, db_begin, db_end, the query of every hit and one partial list */
static inline int64_t sa_batch_per_query_fit(int64_t n, bool hits, int32_t k) { return 8 * n + (hits ? 32 * (int64_t)k : 0); }

/* three quarters of the free memory, under the cap when there is one (cap <= 0: none) */
static inline int64_t sa_batch_budget(uint64_t free_bytes, int64_t cap)
{
	const int64_t budget = (int64_t)(free_bytes - free_bytes / 4);
	return cap > 0 && cap < budget ? cap : budget;
}

/* queries per batch: what the budget holds, one at least, M at most */
static inline int32_t sa_batch_queries(int64_t m, int64_t budget, int64_t per_query)
{
	int64_t nqb = budget / per_query;
	if (nqb > m)
		nqb = m;
	return (int32_t)(nqb < 1 ? 1 : nqb);
}

/* the batches tile [0, M) in order: batch b is [b nqb, b nqb + sa_batch_nq), only the last may be short */
static inline int32_t sa_batch_nq(int64_t m, int32_t nqb, int64_t q0) { return (int32_t)(m - q0 < nqb ? m - q0 : nqb); }
static inline int64_t sa_batch_count(int64_t m, int32_t nqb) { return (m + nqb - 1) / nqb; }

#endif /* SA_SEARCH_BATCH_CORE_H */
