/* search_batch_test.cpp -- the batch rule of the one-call search forms (sequencealigner_amd/csrc/sa_search_batch_core.h) under
 * ASan / UBSan: the bytes of a query, form by form, against the formulas of include/seqalign_hip.h written out; the batch size
 * at its edges; the batches tiling [0, M); and the largest sizes, where UBSan is the judge.  Built and run by
 * tests/test_search_batch_core.py.
 *
 *   search_batch_test --bytes     every form and kind over a sweep of (N, M, k)
 *   search_batch_test --batches   sa_batch_budget / sa_batch_queries at their edges, the tiling for each
 *   search_batch_test --limits    N = M = 2^31 - 1, k = 64, a budget of 2^62
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sequencealigner_amd/csrc/sa_search_batch_core.h"

#define CHECK(c, ...) \
	do { \
		if (!(c)) { \
			fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); \
			fprintf(stderr, __VA_ARGS__); \
			fprintf(stderr, "\n"); \
			exit(1); \
		} \
	} while (0)

static int64_t per_query(int64_t n, int64_t m, bool aligned, bool quantity, bool strands, int64_t tail)
{
	const struct sa_batch_form f = { aligned, quantity, strands, tail };
	return sa_batch_per_query(n, m, f);
}

/* the header's wording, literally; kind 0: raw scores, 1: normalised scores, 2: percent identity */
static void check_bytes(int64_t N, int64_t M, int32_t k)
{
	const int64_t W = (N + 63) / 64;
	for (int hits = 0; hits < 2; hits++) {
		/* sa_hip_search: range row + rectangle row + hits + one partial list */
		CHECK(per_query(N, M, true, false, false, sa_batch_tail_topk(hits, false, false, k)) == 4 * (N + M) + 4 * N + (hits ? 16 * (int64_t)k : 0), "sa_hip_search");
		/* sa_hip_search_norm / _pid: 4 (N + M) bytes (norm only) + 8 N + 20 k (with hits) */
		CHECK(per_query(N, M, true, true, false, sa_batch_tail_topk(hits, true, false, k)) == 4 * (N + M) + 8 * N + (hits ? 20 * (int64_t)k : 0), "sa_hip_search_norm");
		CHECK(per_query(N, M, false, true, false, sa_batch_tail_topk(hits, true, false, k)) == 8 * N + (hits ? 20 * (int64_t)k : 0), "sa_hip_search_pid");
		/* sa_hip_search_strands: 4 (N + 2 M) (not under percent identity) + 8 N (raw) or 16 N (a quantity) + 8 ((N + 63) / 64) + 21 k (with hits) */
		CHECK(per_query(N, M, true, false, true, sa_batch_tail_topk(hits, false, true, k)) == 4 * (N + 2 * M) + 8 * N + 8 * W + (hits ? 21 * (int64_t)k : 0),
		      "sa_hip_search_strands, raw");
		CHECK(per_query(N, M, true, true, true, sa_batch_tail_topk(hits, true, true, k)) == 4 * (N + 2 * M) + 16 * N + 8 * W + (hits ? 21 * (int64_t)k : 0),
		      "sa_hip_search_strands, norm");
		CHECK(per_query(N, M, false, true, true, sa_batch_tail_topk(hits, true, true, k)) == 16 * N + 8 * W + (hits ? 21 * (int64_t)k : 0),
		      "sa_hip_search_strands, pid");
		/* sa_hip_search_fit: a query costs 8 N + 32 k bytes, ranked by the score or not */
		CHECK(sa_batch_per_query_fit(N, hits, k) == 8 * N + (hits ? 32 * (int64_t)k : 0), "sa_hip_search_fit");
	}
	/* sa_hip_search_above: 4 (N + M) (not under percent identity) + 4 N (raw scores) or 8 N, + 8 */
	CHECK(per_query(N, M, true, false, false, sa_batch_tail_above()) == 4 * (N + M) + 4 * N + 8, "sa_hip_search_above, raw");
	CHECK(per_query(N, M, true, true, false, sa_batch_tail_above()) == 4 * (N + M) + 8 * N + 8, "sa_hip_search_above, norm");
	CHECK(per_query(N, M, false, true, false, sa_batch_tail_above()) == 8 * N + 8, "sa_hip_search_above, pid");
	/* sa_hip_search_above_strands: 4 (N + 2 M) (not under percent identity) + 8 N (raw) or 16 N (a quantity) + 8 ((N + 63) / 64) + 8 */
	CHECK(per_query(N, M, true, false, true, sa_batch_tail_above()) == 4 * (N + 2 * M) + 8 * N + 8 * W + 8, "sa_hip_search_above_strands, raw");
	CHECK(per_query(N, M, true, true, true, sa_batch_tail_above()) == 4 * (N + 2 * M) + 16 * N + 8 * W + 8, "sa_hip_search_above_strands, norm");
	CHECK(per_query(N, M, false, true, true, sa_batch_tail_above()) == 16 * N + 8 * W + 8, "sa_hip_search_above_strands, pid");
}

static int do_bytes()
{
	const int64_t ns[] = { 1, 2, 63, 64, 65, 127, 128, 129, 1000, 1000003 }, ms[] = { 1, 3, 7, 4096 };
	const int32_t ks[] = { 1, 5, 64 };
	int cases = 0;
	for (int64_t n : ns)
		for (int64_t m : ms)
			for (int32_t k : ks) {
				check_bytes(n, m, k);
				cases++;
			}
	printf("bytes ok: %d (N, M, k)\n", cases);
	return 0;
}

/* the batches tile [0, M) once, in order; only the last may be short */
static void check_tiling(int64_t m, int32_t nqb)
{
	CHECK(nqb >= 1 && nqb <= m, "nqb = %d of M = %lld", nqb, (long long)m);
	int64_t at = 0, batches = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = sa_batch_nq(m, nqb, q0);
		CHECK(q0 == at, "batch %lld begins at %lld, the one before ended at %lld", (long long)batches, (long long)q0, (long long)at);
		CHECK(nq >= 1 && nq <= nqb, "batch %lld has %d queries", (long long)batches, nq);
		CHECK(nq == nqb || q0 + nq == m, "batch %lld is short and not the last", (long long)batches);
		at = q0 + nq;
		batches++;
	}
	CHECK(at == m, "the batches end at %lld of %lld", (long long)at, (long long)m);
	CHECK(batches == sa_batch_count(m, nqb), "%lld batches, sa_batch_count says %lld", (long long)batches, (long long)sa_batch_count(m, nqb));
}

static int do_batches()
{
	const int64_t per = per_query(1000, 7, true, true, false, sa_batch_tail_topk(true, true, false, 5)); /* 4 * 1007 + 8000 + 100 */
	CHECK(per == 12128, "per query %lld", (long long)per);
	const int64_t m = 7;
	/* budget < per_query: one query per batch */
	CHECK(sa_batch_queries(m, per - 1, per) == 1, "a budget below one query");
	CHECK(sa_batch_queries(m, 0, per) == 1, "no budget");
	check_tiling(m, 1);
	/* an exact multiple, and one byte less */
	CHECK(sa_batch_queries(m, 3 * per, per) == 3, "an exact multiple");
	CHECK(sa_batch_queries(m, 3 * per - 1, per) == 2, "one byte less than an exact multiple");
	check_tiling(m, 3); /* 3, 3, 1 */
	check_tiling(m, 2); /* 2, 2, 2, 1 */
	CHECK(sa_batch_count(m, 3) == 3 && sa_batch_count(m, 2) == 4, "batch counts");
	/* M smaller than budget / per_query */
	CHECK(sa_batch_queries(m, 1000 * per, per) == 7, "more room than queries");
	check_tiling(m, 7);
	CHECK(sa_batch_count(m, 7) == 1, "one batch");
	/* the budget: three quarters of the free bytes; cap 0: uncapped; a cap above the free memory changes nothing */
	const uint64_t free_b = 1000003;
	CHECK(sa_batch_budget(free_b, 0) == 750003, "uncapped: %lld", (long long)sa_batch_budget(free_b, 0));
	CHECK(sa_batch_budget(free_b, -1) == 750003, "a negative cap is none");
	CHECK(sa_batch_budget(free_b, 2000000) == 750003, "a cap above the free memory");
	CHECK(sa_batch_budget(free_b, 750004) == 750003, "a cap above the budget");
	CHECK(sa_batch_budget(free_b, 750002) == 750002, "a cap below the budget");
	CHECK(sa_batch_budget(free_b, 1) == 1, "a cap of one byte");
	CHECK(sa_batch_budget(0, 0) == 0, "no free memory");
	/* the rule end to end, as the GPU tests force batch counts: a cap of 2 queries' bytes over 7 queries is 4 batches */
	const int32_t nqb = sa_batch_queries(m, sa_batch_budget((uint64_t)1 << 38, 2 * per), per);
	CHECK(nqb == 2 && sa_batch_count(m, nqb) == 4, "capped: %d per batch", nqb);
	for (int64_t mm = 1; mm <= 40; mm++)
		for (int32_t q = 1; q <= mm; q++)
			check_tiling(mm, q);
	printf("batches ok\n");
	return 0;
}

static int do_limits()
{
	const int64_t big = 2147483647;
	check_bytes(big, big, 64);
	const int64_t budget = sa_batch_budget(((uint64_t)1 << 62) / 3 * 4 + 4, 0);
	CHECK(budget >= (int64_t)1 << 62, "budget %lld", (long long)budget);
	CHECK(sa_batch_budget(UINT64_MAX / 2, 0) > 0, "the largest free memory an int64 budget holds");
	for (int strands = 0; strands < 2; strands++) {
		const int64_t per = per_query(big, big, true, true, strands, sa_batch_tail_topk(true, true, strands, 64));
		CHECK(per > 0, "per query %lld", (long long)per);
		const int32_t nqb = sa_batch_queries(big, (int64_t)1 << 62, per);
		CHECK(nqb >= 1 && nqb <= big && nqb == (int32_t)(((int64_t)1 << 62) / per), "nqb %d", nqb);
		CHECK(sa_batch_nq(big, nqb, 0) == nqb, "the first batch");
		const int64_t batches = sa_batch_count(big, nqb), last = (batches - 1) * nqb;
		CHECK(last < big && last + sa_batch_nq(big, nqb, last) == big, "the last batch begins at %lld", (long long)last);
		CHECK(sa_batch_queries(big, 0, per) == 1 && sa_batch_count(big, 1) == big, "one query per batch");
	}
	/* a tiny query cost and the largest budget: M bounds the batch */
	CHECK(sa_batch_queries(big, INT64_MAX, 1) == big, "M bounds the batch");
	printf("limits ok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--bytes"))
		return do_bytes();
	if (argc == 2 && !strcmp(argv[1], "--batches"))
		return do_batches();
	if (argc == 2 && !strcmp(argv[1], "--limits"))
		return do_limits();
	fprintf(stderr, "usage: search_batch_test --bytes | --batches | --limits\n");
	return 2;
}
