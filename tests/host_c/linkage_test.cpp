/* linkage_test.cpp -- the contract of the single-linkage tree (sequencealigner_amd/csrc/sa_linkage_core.h) on the host, built
 * with -fsanitize=address,undefined by tests/test_linkage_core.py.
 *
 *   linkage_test --index                the order predicate; the packed index and its inverse up to N = 300 000 (64-bit)
 *   linkage_test --tree SEED N SPREAD   a random packed matrix of N sequences whose scores take SPREAD distinct values (1: all
 *                                       equal): sa_lk_tree_serial against a brute-force Kruskal over every pair
 *   linkage_test --rounds SEED N SPREAD the root rule: Boruvka rounds simulated with sa_lk_before / sa_lk_parent exactly as the
 *                                       kernels run them (best pair per component, hook, mutual pairs once, relabel by walking
 *                                       the parents) against the serial tree; no walk may exceed N steps
 *   linkage_test --cut SEED N SPREAD    sa_lk_labels and sa_lk_merges of the serial tree against double loops over the full
 *                                       matrix, at seven thresholds: below the minimum, the minimum, the median, the maximum,
 *                                       above it, INT32_MIN and INT32_MAX
 *   linkage_test --refuse               trees that are none: a cycle, lo >= hi, an index out of range, scores out of order
 */
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <tuple>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_linkage_core.h"

static int index_check()
{
	const int64_t rows[] = { 0, 1, 2, 3, 63, 64, 65, 4095, 65535, 65536, 89999, 92682, 92683, 92684, 299999, 300000 };
	for (int64_t r : rows)
		for (int64_t c : rows) {
			if (c == r)
				continue;
			const int64_t i = std::min(r, c), j = std::max(r, c), want = j * (j - 1) / 2 + i;
			int64_t lo = -1, hi = -1;
			sa_lk_unpack(sa_lk_packed_at(r, c), &lo, &hi);
			if (sa_lk_packed_at(r, c) != want || lo != i || hi != j) {
				printf("pair (%lld, %lld): index %lld, definition %lld, back (%lld, %lld)\n", (long long)r, (long long)c,
				       (long long)sa_lk_packed_at(r, c), (long long)want, (long long)lo, (long long)hi);
				return 1;
			}
		}
	/* every column's first and last row, where the inverse's square root sits on an edge */
	for (int64_t j = 1; j <= 300000; j++)
		for (int64_t i : { (int64_t)0, j - 1 }) {
			int64_t lo = -1, hi = -1;
			sa_lk_unpack(j * (j - 1) / 2 + i, &lo, &hi);
			if (lo != i || hi != j) {
				printf("unpack(%lld) = (%lld, %lld), want (%lld, %lld)\n", (long long)(j * (j - 1) / 2 + i), (long long)lo, (long long)hi,
				       (long long)i, (long long)j);
				return 1;
			}
		}
	const int64_t big = (int64_t)5000000000;
	const bool ok = sa_lk_before(5, 9, 4, 0) && !sa_lk_before(4, 0, 5, 9) && sa_lk_before(5, 3, 5, 4) && !sa_lk_before(5, 4, 5, 3) &&
			!sa_lk_before(5, 3, 5, 3) && sa_lk_before(INT32_MAX, big, INT32_MIN, 0) && !sa_lk_before(INT32_MIN, 0, INT32_MAX, big) &&
			sa_lk_before(INT32_MIN, big - 1, INT32_MIN, big) && sa_lk_before(0, (int64_t)1 << 32, -1, 0) &&
			sa_lk_before(7, ((int64_t)1 << 32) - 1, 7, (int64_t)1 << 32);
	if (!ok) {
		printf("predicate wrong\n");
		return 1;
	}
	printf("index ok\n");
	return 0;
}

struct Case {
	int32_t num;
	std::vector<int32_t> packed; /* (exactly as long as the packed matrix: ASan sees any index beyond it) */
	std::vector<int32_t> full;
};

static Case make_case(unsigned seed, int32_t num, int32_t spread)
{
	Case k;
	k.num = num;
	std::mt19937 rng(seed);
	const size_t n = (size_t)num;
	k.packed.resize(n * (n - 1) / 2);
	for (int32_t &v : k.packed)
		v = (int32_t)(rng() % (uint32_t)spread) - spread / 2;
	k.full.assign(n * n, 0);
	for (size_t j = 1; j < n; j++)
		for (size_t i = 0; i < j; i++)
			k.full[i * n + j] = k.full[j * n + i] = k.packed[j * (j - 1) / 2 + i];
	return k;
}

/* the definition, from the full matrix: every pair sorted by (score descending, packed index ascending), joined iff its ends
 * are in different components; components by relabelling in a loop, no union-find */
static void kruskal(const Case &k, std::vector<int32_t> &pairs, std::vector<int32_t> &score)
{
	const size_t n = (size_t)k.num;
	std::vector<std::tuple<int64_t, int64_t, int32_t, int32_t>> all;
	for (size_t j = 1; j < n; j++)
		for (size_t i = 0; i < j; i++)
			all.emplace_back(-(int64_t)k.full[i * n + j], (int64_t)(j * (j - 1) / 2 + i), (int32_t)i, (int32_t)j);
	std::sort(all.begin(), all.end());
	std::vector<int32_t> comp(n);
	for (size_t v = 0; v < n; v++)
		comp[v] = (int32_t)v;
	for (const auto &[neg, p, i, j] : all) {
		(void)p;
		const int32_t a = comp[(size_t)i], b = comp[(size_t)j];
		if (a == b)
			continue;
		for (int32_t &c : comp)
			if (c == b)
				c = a;
		pairs.push_back(i);
		pairs.push_back(j);
		score.push_back((int32_t)-neg);
	}
}

static int tree(unsigned seed, int32_t num, int32_t spread)
{
	const Case k = make_case(seed, num, spread);
	const size_t m = (size_t)num - 1;
	std::vector<int32_t> pairs(2 * m, -7), score(m, -7), want_pairs, want_score;
	if (sa_lk_tree_serial(k.packed.data(), num, pairs.data(), score.data())) {
		printf("sa_lk_tree_serial failed\n");
		return 1;
	}
	kruskal(k, want_pairs, want_score);
	if (want_score.size() != m || pairs != want_pairs || score != want_score) {
		printf("the serial tree differs from Kruskal's\n");
		return 1;
	}
	printf("tree ok: %d rows, %zu merges\n", num, m);
	return 0;
}

/* the rounds as the kernels run them */
static int rounds(unsigned seed, int32_t num, int32_t spread)
{
	const Case k = make_case(seed, num, spread);
	const size_t n = (size_t)num, m = n - 1;
	std::vector<int32_t> comp(n), parent(n), es(n, 0), vscore(n), cbest(n);
	std::vector<int64_t> ep(n, -1), vp(n), cp(n);
	std::vector<char> chas(n);
	for (size_t v = 0; v < n; v++)
		comp[v] = (int32_t)v;
	int taken = 0, mutual = 0, deepest = 0;
	for (;;) {
		bool more = false;
		for (size_t v = 0; v < n; v++)
			more |= comp[v] != comp[0];
		if (!more)
			break;
		taken++;
		for (size_t v = 0; v < n; v++) {
			parent[v] = (int32_t)v;
			chas[v] = 0;
			cp[v] = -1;
			vp[v] = -1;
		}
		for (size_t r = 0; r < n; r++) /* best */
			for (size_t c = 0; c < n; c++) {
				if (c == r || comp[c] == comp[r])
					continue;
				const int64_t p = sa_lk_packed_at((int64_t)r, (int64_t)c);
				if (vp[r] < 0 || sa_lk_before(k.packed[(size_t)p], p, vscore[r], vp[r])) {
					vscore[r] = k.packed[(size_t)p];
					vp[r] = p;
				}
			}
		for (size_t v = 0; v < n; v++) { /* the maximum of the score ... */
			const size_t c = (size_t)comp[v];
			if (vp[v] >= 0 && (!chas[c] || vscore[v] > cbest[c])) {
				chas[c] = 1;
				cbest[c] = vscore[v];
			}
		}
		for (size_t v = 0; v < n; v++) { /* ... then the minimum of p among the vertices that hold it */
			const size_t c = (size_t)comp[v];
			if (vp[v] >= 0 && vscore[v] == cbest[c] && (cp[c] < 0 || vp[v] < cp[c]))
				cp[c] = vp[v];
		}
		for (size_t c = 0; c < n; c++) { /* hook */
			if (comp[c] != (int32_t)c || cp[c] < 0)
				continue;
			int64_t lo, hi;
			sa_lk_unpack(cp[c], &lo, &hi);
			const int32_t a = comp[(size_t)lo], b = comp[(size_t)hi];
			if ((a == (int32_t)c) == (b == (int32_t)c)) {
				printf("component %zu: its pair does not leave it\n", c);
				return 1;
			}
			const int32_t d = a == (int32_t)c ? b : a;
			const int32_t up = sa_lk_parent((int32_t)c, d, cp[c], cp[(size_t)d]);
			if (cp[(size_t)d] == cp[c]) {
				mutual++;
				if (up != std::min((int32_t)c, d) || sa_lk_parent(d, (int32_t)c, cp[(size_t)d], cp[c]) != up) {
					printf("mutual pair %zu / %d: the smaller id must stay the root\n", c, d);
					return 1;
				}
			} else if (up != d) {
				printf("component %zu must hook to %d\n", c, d);
				return 1;
			}
			parent[c] = up;
			if (up != (int32_t)c) {
				if (ep[c] >= 0) {
					printf("slot %zu is written twice\n", c);
					return 1;
				}
				ep[c] = cp[c];
				es[c] = cbest[c];
			}
		}
		for (size_t v = 0; v < n; v++) { /* relabel */
			int32_t c = comp[v];
			int steps = 0;
			while (parent[(size_t)c] != c) {
				c = parent[(size_t)c];
				if (++steps > num) {
					printf("a walk along the parents does not end: a cycle\n");
					return 1;
				}
			}
			deepest = std::max(deepest, steps);
			comp[v] = c;
		}
		if (taken > 32) {
			printf("more than 32 rounds\n");
			return 1;
		}
	}
	int bound = 0;
	while (((int64_t)1 << bound) < num)
		bound++;
	if (taken > bound) {
		printf("%d rounds, the bound is %d\n", taken, bound);
		return 1;
	}
	/* the slots, ranked by counting */
	std::vector<int32_t> pairs(2 * m, -7), score(m, -7), want_pairs(2 * m), want_score(m);
	size_t filled = 0;
	for (size_t v = 0; v < n; v++) {
		if (ep[v] < 0)
			continue;
		filled++;
		size_t rank = 0;
		for (size_t u = 0; u < n; u++)
			rank += ep[u] >= 0 && sa_lk_before(es[u], ep[u], es[v], ep[v]);
		int64_t lo, hi;
		sa_lk_unpack(ep[v], &lo, &hi);
		if (rank >= m) {
			printf("rank %zu of %zu\n", rank, m);
			return 1;
		}
		pairs[2 * rank] = (int32_t)lo;
		pairs[2 * rank + 1] = (int32_t)hi;
		score[rank] = es[v];
	}
	sa_lk_tree_serial(k.packed.data(), num, want_pairs.data(), want_score.data());
	if (filled != m || pairs != want_pairs || score != want_score) {
		printf("the rounds give another tree than Prim (%zu of %zu slots filled)\n", filled, m);
		return 1;
	}
	printf("rounds ok: %d rows, %d rounds (bound %d), %d mutual hooks, deepest chain %d\n", num, taken, bound, mutual, deepest);
	return 0;
}

static int cut(unsigned seed, int32_t num, int32_t spread)
{
	const Case k = make_case(seed, num, spread);
	const size_t n = (size_t)num, m = n - 1;
	std::vector<int32_t> pairs(2 * m), score(m);
	sa_lk_tree_serial(k.packed.data(), num, pairs.data(), score.data());
	std::vector<int32_t> sorted(k.packed);
	std::sort(sorted.begin(), sorted.end());
	const int32_t lo = sorted.front(), hi = sorted.back(), mid = sorted[sorted.size() / 2];
	const int32_t thresholds[] = { lo - 1, lo, mid, hi, hi + 1, INT32_MIN, INT32_MAX };
	for (int32_t t : thresholds) {
		/* components of the graph score >= t by flooding from the smallest unlabelled index */
		std::vector<int32_t> want(n, -1), stack;
		int32_t clusters = 0;
		for (size_t r = 0; r < n; r++) {
			if (want[r] >= 0)
				continue;
			clusters++;
			want[r] = (int32_t)r;
			stack.push_back((int32_t)r);
			while (!stack.empty()) {
				const size_t v = (size_t)stack.back();
				stack.pop_back();
				for (size_t c = 0; c < n; c++)
					if (c != v && want[c] < 0 && k.full[v * n + c] >= t) {
						want[c] = (int32_t)r;
						stack.push_back((int32_t)c);
					}
			}
		}
		if ((t <= lo && clusters != 1) || (t > hi && clusters != num)) {
			printf("T = %d: the flood itself is off (%d clusters)\n", t, clusters);
			return 1;
		}
		std::vector<int32_t> labels(n, -7);
		const int32_t got = sa_lk_labels(pairs.data(), score.data(), num, t, labels.data());
		if (got != clusters || labels != want) {
			printf("T = %d: %d clusters, want %d; labels %s\n", t, got, clusters, labels == want ? "equal" : "differ");
			return 1;
		}
	}
	/* the merge table by relabelling every member in a loop */
	std::vector<int32_t> id(n), left(m, -7), right(m, -7), size(m, -7);
	for (size_t v = 0; v < n; v++)
		id[v] = (int32_t)v;
	if (sa_lk_merges(pairs.data(), num, left.data(), right.data(), size.data())) {
		printf("sa_lk_merges failed\n");
		return 1;
	}
	for (size_t t = 0; t < m; t++) {
		const int32_t a = id[(size_t)pairs[2 * t]], b = id[(size_t)pairs[2 * t + 1]];
		int32_t members = 0;
		for (int32_t &c : id)
			if (c == a || c == b) {
				c = num + (int32_t)t;
				members++;
			}
		if (a == b || left[t] != std::min(a, b) || right[t] != std::max(a, b) || size[t] != members) {
			printf("merge %zu: (%d, %d, %d), want (%d, %d, %d)\n", t, left[t], right[t], size[t], std::min(a, b), std::max(a, b), members);
			return 1;
		}
	}
	if (m && size[m - 1] != num) {
		printf("the last merge holds %d of %d sequences\n", size[m - 1], num);
		return 1;
	}
	printf("cut ok: %d rows, %zu thresholds, %zu merges\n", num, sizeof(thresholds) / sizeof(thresholds[0]), m);
	return 0;
}

static int refuse()
{
	const int32_t num = 5;
	const int32_t good_pairs[] = { 0, 1, 2, 3, 1, 2, 3, 4 }, good_score[] = { 9, 9, 4, -3 };
	int32_t labels[5], left[4], right[4], size[4];
	auto untouched = [&] {
		for (int t = 0; t < 5; t++)
			if (labels[t] != -7)
				return false;
		for (int t = 0; t < 4; t++)
			if (left[t] != -7 || right[t] != -7 || size[t] != -7)
				return false;
		return true;
	};
	auto poison = [&] {
		std::fill(labels, labels + 5, -7);
		std::fill(left, left + 4, -7);
		std::fill(right, right + 4, -7);
		std::fill(size, size + 4, -7);
	};
	struct Bad {
		const char *what;
		int32_t pairs[8], score[4];
		int code;
		bool merges_too; /* (the merge table has no scores to check) */
	} bad[] = {
		{ "a cycle", { 0, 1, 1, 2, 0, 2, 3, 4 }, { 9, 8, 7, 6 }, SA_LK_CYCLE, true },
		{ "lo > hi", { 1, 0, 2, 3, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_LO_HI, true },
		{ "lo == hi", { 0, 1, 2, 2, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_LO_HI, true },
		{ "an index of N", { 0, 1, 2, 3, 1, 2, 3, 5 }, { 9, 9, 4, -3 }, SA_LK_RANGE, true },
		{ "a negative index", { 0, 1, -1, 3, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_RANGE, true },
		{ "scores ascending", { 0, 1, 2, 3, 1, 2, 3, 4 }, { 9, 9, 4, 5 }, SA_LK_ORDER, false },
		{ "equal scores, packed index descending", { 2, 3, 0, 1, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_ORDER, false },
	};
	for (const Bad &b : bad) {
		poison();
		const int32_t got = sa_lk_labels(b.pairs, b.score, num, 0, labels);
		const int got_m = b.merges_too ? sa_lk_merges(b.pairs, num, left, right, size) : b.code;
		if (got != b.code || got_m != b.code || !untouched()) {
			printf("%s: labels %d, merges %d, want %d; outputs %s\n", b.what, got, got_m, b.code, untouched() ? "untouched" : "WRITTEN");
			return 1;
		}
	}
	poison();
	if (sa_lk_labels(good_pairs, good_score, num, 5, labels) != 3 || labels[0] != 0 || labels[1] != 0 || labels[2] != 2 || labels[3] != 2 ||
	    labels[4] != 4 || sa_lk_merges(good_pairs, num, left, right, size) || left[2] != 5 || right[2] != 6 || size[2] != 4 || left[3] != 4 ||
	    right[3] != 7 || size[3] != 5) {
		printf("the good tree is refused or read wrongly\n");
		return 1;
	}
	int32_t one = -7;
	if (sa_lk_labels(nullptr, nullptr, 1, 0, &one) != 1 || one != 0) {
		printf("one sequence is one cluster\n");
		return 1;
	}
	printf("refuse ok: %zu trees\n", sizeof(bad) / sizeof(bad[0]));
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--index"))
		return index_check();
	if (argc == 2 && !strcmp(argv[1], "--refuse"))
		return refuse();
	if (argc == 5 && atoi(argv[3]) >= 2 && atoi(argv[4]) >= 1) {
		const unsigned seed = (unsigned)atoi(argv[2]);
		const int32_t num = atoi(argv[3]), spread = atoi(argv[4]);
		if (!strcmp(argv[1], "--tree"))
			return tree(seed, num, spread);
		if (!strcmp(argv[1], "--rounds"))
			return rounds(seed, num, spread);
		if (!strcmp(argv[1], "--cut"))
			return cut(seed, num, spread);
	}
	printf("usage: linkage_test --index | --refuse | --tree SEED N SPREAD | --rounds SEED N SPREAD | --cut SEED N SPREAD\n");
	return 2;
}
