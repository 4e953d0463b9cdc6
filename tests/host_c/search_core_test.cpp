/* search_core_test.cpp -- the host-compilable core of the search (sequencealigner_amd/csrc/sa_search_core.h) under ASan /
 * UBSan: segment bounds, segment counts, range offsets and the serial part + merge selection of the hits against
 * std::partial_sort.  Built and run by tests/test_search_core.py.
 *
 *   search_core_test --select N K S SPREAD   one rectangle of 6 rows x N, scores in [0, SPREAD); prints
 *                                            "select ok: 6 rows, N = .., k = .., S = .., T rows with a tie across the cut"
 *   search_core_test --segments              bounds cover [0, N) once for every (N, S) of a sweep, S > N included
 *   search_core_test --counts                sa_hits_segments: limits and the cases the GPU tests name
 *   search_core_test --offsets               sa_search_row_at / sa_search_range_elems against a running sum, past 2^32
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_search_core.h"

#define CHECK(c, ...) \
	do { \
		if (!(c)) { \
			fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); \
			fprintf(stderr, __VA_ARGS__); \
			fprintf(stderr, "\n"); \
			exit(1); \
		} \
	} while (0)

static int do_select(int32_t n, int32_t k, int32_t S, int32_t spread)
{
	CHECK(n >= 1 && k >= 1 && k <= 64 && k <= n && S >= 1 && spread >= 1, "bad arguments");
	const int rows = 6;
	std::mt19937 rng(12345u + (unsigned)n * 7u + (unsigned)k * 131u + (unsigned)S * 17u + (unsigned)spread);
	std::vector<int32_t> rect((size_t)rows * (size_t)n);
	for (auto &v : rect)
		v = (int32_t)(rng() % (unsigned)spread) - spread / 2; /* (negative scores too) */
	std::vector<uint64_t> part((size_t)S * (size_t)k);
	std::vector<int32_t> index((size_t)k), score((size_t)k), order((size_t)n);
	int ties = 0;
	for (int r = 0; r < rows; r++) {
		const int32_t *row = rect.data() + (size_t)r * (size_t)n;
		sa_hits_select_row(row, n, k, S, part.data(), index.data(), score.data());
		for (int32_t d = 0; d < n; d++)
			order[(size_t)d] = d;
		std::partial_sort(order.begin(), order.begin() + k, order.end(),
				  [&](int32_t a, int32_t b) { return row[a] != row[b] ? row[a] > row[b] : a < b; });
		for (int32_t t = 0; t < k; t++) {
			CHECK(index[(size_t)t] == order[(size_t)t], "row %d entry %d: index %d, expected %d", r, t, index[(size_t)t], order[(size_t)t]);
			CHECK(score[(size_t)t] == row[order[(size_t)t]], "row %d entry %d: score %d, expected %d", r, t, score[(size_t)t], row[order[(size_t)t]]);
		}
		if (k < n) {
			std::nth_element(order.begin() + k, order.begin() + k, order.end(),
					 [&](int32_t a, int32_t b) { return row[a] != row[b] ? row[a] > row[b] : a < b; });
			ties += row[order[(size_t)k]] == row[order[(size_t)k - 1]];
		}
	}
	printf("select ok: %d rows, N = %d, k = %d, S = %d, %d rows with a tie across the cut\n", rows, n, k, S, ties);
	return 0;
}

static int do_segments()
{
	const int32_t ns[] = { 1, 2, 63, 64, 65, 1000, 200000, INT32_MAX };
	const int32_t ss[] = { 1, 2, 5, 64, 1000, 1024, 70000 };
	long cases = 0;
	for (int32_t n : ns)
		for (int32_t S : ss) {
			CHECK(sa_hits_seg_begin(n, S, 0) == 0 && sa_hits_seg_begin(n, S, S) == n, "ends of N = %d, S = %d", n, S);
			int64_t covered = 0;
			for (int32_t s = 0; s < S; s++) {
				const int32_t a = sa_hits_seg_begin(n, S, s), b = sa_hits_seg_begin(n, S, s + 1);
				CHECK(a <= b && a >= 0 && b <= n, "segment %d of N = %d, S = %d: [%d, %d)", s, n, S, a, b);
				covered += b - a;
			}
			CHECK(covered == n, "N = %d, S = %d: %lld covered", n, S, (long long)covered);
			cases++;
		}
	/* every candidate in exactly one segment, S > N included */
	for (int32_t n : { 1, 5, 65 })
		for (int32_t S : { 1, 2, 5, n, n + 1, 3 * n + 1 }) {
			std::vector<int> seen((size_t)n, 0);
			for (int32_t s = 0; s < S; s++)
				for (int32_t d = sa_hits_seg_begin(n, S, s); d < sa_hits_seg_begin(n, S, s + 1); d++)
					seen[(size_t)d]++;
			for (int32_t d = 0; d < n; d++)
				CHECK(seen[(size_t)d] == 1, "N = %d, S = %d: candidate %d in %d segments", n, S, d, seen[(size_t)d]);
			cases++;
		}
	printf("segments ok: %ld cases\n", cases);
	return 0;
}

static int do_counts()
{
	for (int32_t n : { 1, 15, 16, 65, 1000, 200000, 1000000, INT32_MAX })
		for (int32_t nq : { 1, 2, 3, 10, 2047, 2048, 3000, 1000000, INT32_MAX })
			for (int32_t k : { 1, 7, 64 }) {
				const int32_t S = sa_hits_segments(n, nq, k);
				CHECK(S >= 1 && S <= SA_HITS_SEG_MAX, "S = %d", S);
				if (S > 1) {
					CHECK(nq < SA_HITS_ROWS_FILL, "split with %d rows", nq);
					CHECK((int64_t)S * std::max(4 * k, SA_HITS_SEG_MIN) <= n, "N = %d, k = %d: S = %d leaves too short segments", n, k, S);
					CHECK((int64_t)nq * (S - 1) < SA_HITS_WAVES, "N = %d, nq = %d: S = %d is more than fills the device", n, nq, S);
				}
			}
	/* the cases tests/test_gpu_search.py names */
	CHECK(sa_hits_segments(200000, 2, 1) == SA_HITS_SEG_MAX && sa_hits_segments(200000, 2, 64) == 200000 / 256, "(2, 200000)");
	CHECK(sa_hits_segments(65, 3, 1) == 4 && sa_hits_segments(65, 3, 7) == 2 && sa_hits_segments(65, 3, 64) == 1, "(3, 65)");
	CHECK(sa_hits_segments(70, 3000, 1) == 1 && sa_hits_segments(70, 3000, 64) == 1, "(3000, 70)");
	CHECK(sa_hits_segments(1, 5, 1) == 1, "(5, 1)");
	printf("counts ok\n");
	return 0;
}

static int do_offsets()
{
	for (int64_t n : { (int64_t)1, (int64_t)700, (int64_t)100000 })
		for (int64_t q0 : { (int64_t)0, (int64_t)17, (int64_t)90000 }) {
			int64_t at = 0;
			for (int64_t q = q0; q < q0 + 70; q++) {
				CHECK(sa_search_row_at(n, q0, q) == at, "N = %lld, q0 = %lld, q = %lld", (long long)n, (long long)q0, (long long)q);
				at += n + q; /* column N + q of the concatenated store has N + q rows */
			}
			CHECK(sa_search_range_elems(n, q0, 70) == at, "range of N = %lld, q0 = %lld", (long long)n, (long long)q0);
		}
	CHECK(sa_search_range_elems(100000, 0, 100000) == sa_search_tri(200000) - sa_search_tri(100000), "past 2^32");
	CHECK(sa_search_range_elems(100000, 0, 100000) > ((int64_t)1 << 33), "past 2^32");
	printf("offsets ok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 6 && !strcmp(argv[1], "--select"))
		return do_select(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
	if (argc == 2 && !strcmp(argv[1], "--segments"))
		return do_segments();
	if (argc == 2 && !strcmp(argv[1], "--counts"))
		return do_counts();
	if (argc == 2 && !strcmp(argv[1], "--offsets"))
		return do_offsets();
	fprintf(stderr, "usage: search_core_test --select N K S SPREAD | --segments | --counts | --offsets\n");
	return 2;
}
