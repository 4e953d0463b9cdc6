/* edges_test.cpp -- the contract of the score graph (sequencealigner_amd/csrc/sa_edges_core.h) on the host, built with
 * -fsanitize=address,undefined by tests/test_edges_core.py.
 *
 *   edges_test --index               the packed index of a row's two pieces against the definition (pair i < j at j (j - 1) / 2 + i)
 *   edges_test --graph SEED N SPREAD a random symmetric matrix of N sequences whose scores take SPREAD distinct values (1: all
 *                                    equal): sa_edge_offsets + sa_edge_fill_row of every row against a brute-force double loop
 *                                    over the full matrix, for thresholds below the minimum, at the minimum, at a value that
 *                                    occurs (the median), at the maximum, above it, INT32_MIN and INT32_MAX
 */
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_edges_core.h"

static int index_check()
{
	const int64_t rows[] = { 0, 1, 2, 3, 63, 64, 65, 4095, 89999, 300000 };
	for (int64_t r : rows)
		for (int64_t c : rows) {
			if (c == r)
				continue;
			const int64_t i = std::min(r, c), j = std::max(r, c), want = j * (j - 1) / 2 + i;
			const int64_t got = c < r ? sa_edge_left_at(r, c) : sa_edge_right_at(r, c);
			if (got != want || sa_nb_packed_at(r, c) != want) {
				printf("entry (%lld, %lld): piece index %lld, definition %lld\n", (long long)r, (long long)c, (long long)got, (long long)want);
				return 1;
			}
		}
	/* the left piece is one run, the right piece one element per column with consecutive rows side by side */
	if (sa_edge_left_at(70, 1) != sa_edge_left_at(70, 0) + 1 || sa_edge_right_at(6, 70) != sa_edge_right_at(5, 70) + 1) {
		printf("runs are not contiguous\n");
		return 1;
	}
	if (!sa_edge_pass(5, 5) || sa_edge_pass(4, 5) || !sa_edge_pass(INT32_MIN, INT32_MIN) || sa_edge_pass(INT32_MAX - 1, INT32_MAX) ||
	    !sa_edge_pass(INT32_MAX, INT32_MAX)) {
		printf("predicate wrong\n");
		return 1;
	}
	printf("index ok\n");
	return 0;
}

static int graph(unsigned seed, int32_t num, int32_t spread)
{
	if (num < 2 || spread < 1) {
		printf("bad arguments\n");
		return 2;
	}
	std::mt19937 rng(seed);
	const size_t n = (size_t)num, pairs = n * (n - 1) / 2;
	std::vector<int32_t> packed(pairs); /* (exactly as long as the packed matrix: ASan sees any index beyond it) */
	for (int32_t &v : packed)
		v = (int32_t)(rng() % (uint32_t)spread) - spread / 2;
	/* the full symmetric matrix, from the definition alone */
	std::vector<int32_t> full(n * n, 0);
	for (size_t j = 1; j < n; j++)
		for (size_t i = 0; i < j; i++)
			full[i * n + j] = full[j * n + i] = packed[j * (j - 1) / 2 + i];
	std::vector<int32_t> sorted(packed);
	std::sort(sorted.begin(), sorted.end());
	const int32_t lo = sorted.front(), hi = sorted.back(), mid = sorted[pairs / 2];
	const int32_t thresholds[] = { lo - 1, lo, mid, hi, hi + 1, INT32_MIN, INT32_MAX };
	size_t checked = 0, empty_rows = 0;
	for (int32_t t : thresholds) {
		std::vector<int64_t> want_off(n + 1, 0);
		std::vector<int32_t> want_idx, want_sco;
		for (size_t r = 0; r < n; r++) {
			for (size_t c = 0; c < n; c++)
				if (c != r && full[r * n + c] >= t) {
					want_idx.push_back((int32_t)c);
					want_sco.push_back(full[r * n + c]);
				}
			want_off[r + 1] = (int64_t)want_idx.size();
		}
		if ((t <= lo && want_idx.size() != n * (n - 1)) || (t > hi && !want_idx.empty()) || (t == hi && want_idx.size() < 2)) {
			printf("T = %d: the brute-force loop itself is off (%zu edges)\n", t, want_idx.size());
			return 1;
		}
		std::vector<int64_t> offsets(n + 1, -1);
		sa_edge_offsets(packed.data(), num, t, offsets.data());
		if (offsets != want_off) {
			printf("T = %d: offsets differ\n", t);
			return 1;
		}
		const size_t e = (size_t)offsets[n];
		std::vector<int32_t> index(e), score(e); /* (exactly E elements) */
		for (int32_t r = 0; r < num; r++) {
			const int64_t end = sa_edge_fill_row(packed.data(), num, r, t, offsets[(size_t)r], index.data(), score.data());
			if (end != offsets[(size_t)r + 1] || end - offsets[(size_t)r] != sa_edge_count_row(packed.data(), num, r, t)) {
				printf("T = %d row %d: the fill ends at %lld, the offsets say %lld\n", t, r, (long long)end, (long long)offsets[(size_t)r + 1]);
				return 1;
			}
			empty_rows += end == offsets[(size_t)r];
		}
		if (index != want_idx || score != want_sco) {
			printf("T = %d: index or score differ\n", t);
			return 1;
		}
		if (e % 2) {
			printf("T = %d: E = %zu is odd\n", t, e);
			return 1;
		}
		checked += e;
	}
	printf("graph ok: %d rows, %zu thresholds, %zu edges compared, %zu empty rows met\n", num, sizeof(thresholds) / sizeof(thresholds[0]), checked,
	       empty_rows);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--index"))
		return index_check();
	if (argc == 5 && !strcmp(argv[1], "--graph"))
		return graph((unsigned)atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
	printf("usage: edges_test --index | --graph SEED N SPREAD\n");
	return 2;
}
