/* agglo_test.cpp -- the contract of complete and average linkage (sequencealigner_amd/csrc/sa_agglo_core.h) on the host, built
 * with -fsanitize=address,undefined by tests/test_agglo_core.py.
 *
 *   agglo_test --predicate               the order at the extremes: S = +-(2^62 - 1), n up to 2^34 (128-bit products), equal
 *                                        rationals with different (S, n), antisymmetry and transitivity over a random sample, the
 *                                        floor of negative quotients
 *   agglo_test --index                   the position in the working matrix and the sums at N = 131072
 *   agglo_test --replay SEED N SPREAD M  a random packed matrix of N sequences whose scores take SPREAD distinct values (1: all
 *                                        equal), method M (1 complete, 2 average): the DEVICE's steps -- row-best caches by lanes
 *                                        and a reduction, pick, the merge with sa_ag_cache and its rescans -- replayed with the
 *                                        core functions against sa_ag_tree_serial, and for N <= 65 against a restatement that
 *                                        recomputes every similarity from the members
 *   agglo_test --cut SEED N SPREAD M     sa_ag_labels of the serial tree against a double loop, at seven thresholds
 *   agglo_test --refuse                  trees and score sequences that must be refused, with nothing written
 */
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_agglo_core.h"

typedef __int128 i128;

static int sign(i128 v) { return v > 0 ? 1 : v < 0 ? -1 : 0; }

static int predicate_check()
{
	const int64_t big = ((int64_t)1 << 62) - 1, wide = (int64_t)1 << 34;
	/* the extremes: the products pass 2^96 */
	bool ok = sa_ag_cmp_avg(big, wide, big, wide) == 0 && sa_ag_cmp_avg(big, wide - 1, big, wide) == 1 &&
		  sa_ag_cmp_avg(-big, wide - 1, -big, wide) == -1 && sa_ag_cmp_avg(big, wide, -big, wide) == 1 &&
		  sa_ag_cmp_avg(-big, 1, big, wide) == -1 && sa_ag_cmp_avg(big - 1, wide, big, wide) == -1 &&
		  sa_ag_cmp_avg(big, 1, big, wide) == 1 && sa_ag_cmp_avg(0, wide, 0, 1) == 0;
	/* equal rationals with different (S, n); the packed index then decides */
	ok = ok && sa_ag_cmp_avg(6, 4, 3, 2) == 0 && sa_ag_cmp_avg(-6, 4, -9, 6) == 0 && sa_ag_cmp_avg(((int64_t)1 << 61), wide, ((int64_t)1 << 60), wide / 2) == 0 &&
	     sa_ag_before<SA_AGGLO_AVERAGE>(6, 4, 10, 3, 2, 11) && !sa_ag_before<SA_AGGLO_AVERAGE>(3, 2, 11, 6, 4, 10) &&
	     !sa_ag_before<SA_AGGLO_AVERAGE>(6, 4, 10, 3, 2, 10) && sa_ag_before<SA_AGGLO_AVERAGE>(7, 4, 99, 3, 2, 0) &&
	     sa_ag_before<SA_AGGLO_COMPLETE>(INT32_MAX, 1, (int64_t)5000000000, INT32_MIN, 1, 0) &&
	     sa_ag_before<SA_AGGLO_COMPLETE>(INT32_MIN, 1, 3, INT32_MIN, 1, 4) && !sa_ag_before<SA_AGGLO_COMPLETE>(INT32_MIN, 1, 4, INT32_MIN, 1, 4);
	if (!ok) {
		printf("predicate wrong at the extremes\n");
		return 1;
	}
	std::mt19937_64 rng(12345);
	struct Key {
		int64_t s, n, p;
	};
	std::vector<Key> keys;
	for (int t = 0; t < 600; t++) {
		const int shift = (int)(rng() % 63);
		int64_t s = (int64_t)(rng() >> 1) >> shift;
		if (s > big)
			s = big;
		if (rng() & 1)
			s = -s;
		const int64_t n = 1 + (int64_t)(rng() % (uint64_t)(t % 3 ? wide : 5));
		keys.push_back({ s, n, (int64_t)(rng() % 40) });
		if (t % 5 == 0 && s % 2 == 0 && n % 2 == 0) /* the same rational, other terms */
			keys.push_back({ s / 2, n / 2, (int64_t)(rng() % 40) });
	}
	for (const Key &x : keys)
		for (const Key &y : keys) {
			const int want = sign((i128)x.s * y.n - (i128)y.s * x.n);
			if (sa_ag_cmp_avg(x.s, x.n, y.s, y.n) != want || sa_ag_cmp_avg(y.s, y.n, x.s, x.n) != -want) {
				printf("cmp(%lld / %lld, %lld / %lld) wrong\n", (long long)x.s, (long long)x.n, (long long)y.s, (long long)y.n);
				return 1;
			}
			const bool xy = sa_ag_before<SA_AGGLO_AVERAGE>(x.s, x.n, x.p, y.s, y.n, y.p), yx = sa_ag_before<SA_AGGLO_AVERAGE>(y.s, y.n, y.p, x.s, x.n, x.p);
			if ((xy && yx) || (!xy && !yx && !(want == 0 && x.p == y.p))) {
				printf("not antisymmetric / not total\n");
				return 1;
			}
		}
	for (size_t t = 0; t < 200000; t++) { /* transitivity over random triples */
		const Key &x = keys[rng() % keys.size()], &y = keys[rng() % keys.size()], &z = keys[rng() % keys.size()];
		if (sa_ag_before<SA_AGGLO_AVERAGE>(x.s, x.n, x.p, y.s, y.n, y.p) && sa_ag_before<SA_AGGLO_AVERAGE>(y.s, y.n, y.p, z.s, z.n, z.p) &&
		    !sa_ag_before<SA_AGGLO_AVERAGE>(x.s, x.n, x.p, z.s, z.n, z.p)) {
			printf("not transitive\n");
			return 1;
		}
	}
	/* the floor */
	const int64_t fl[][3] = { { 7, 2, 3 }, { -7, 2, -4 }, { -8, 2, -4 }, { -1, 3, -1 }, { 0, 5, 0 }, { 1, 3, 0 }, { -big, wide, -((big + wide - 1) / wide) },
				  { big, wide, big / wide }, { (int64_t)INT32_MIN * 4, 4, INT32_MIN }, { (int64_t)INT32_MIN * 4 + 1, 4, INT32_MIN },
				  { -1, wide, -1 } };
	for (const auto &f : fl)
		if (sa_ag_floor_div(f[0], f[1]) != f[2]) {
			printf("floor(%lld / %lld) = %lld, want %lld\n", (long long)f[0], (long long)f[1], (long long)sa_ag_floor_div(f[0], f[1]), (long long)f[2]);
			return 1;
		}
	printf("predicate ok: %zu keys\n", keys.size());
	return 0;
}

static int index_check()
{
	const int64_t n = SA_AGGLO_AVERAGE_MAX_NUM;
	bool ok = n == 131072 && sa_ag_at(n - 1, n - 1, n) == ((int64_t)1 << 34) - 1 && sa_ag_at(46341, 0, n) > ((int64_t)1 << 31) &&
		  sa_ag_at(n - 1, 0, n) == (n - 1) * n && sa_lk_packed_at(n - 1, n - 2) == n * (n - 1) / 2 - 1;
	/* the largest sums: two clusters of N / 2 members, every score an extreme */
	const int64_t half = n / 2, cross = half * half;
	const int64_t low = (int64_t)INT32_MIN * cross, high = (int64_t)INT32_MAX * cross; /* -2^63 exactly; no overflow under UBSan */
	ok = ok && low == INT64_MIN && high > 0 && sa_ag_cmp_avg(low, cross, high, cross) == -1 && sa_ag_cmp_avg(low, cross, INT32_MIN, 1) == 0 &&
	     sa_ag_cmp_avg(high, cross, INT32_MAX, 1) == 0 && sa_ag_floor_div(low, cross) == INT32_MIN && sa_ag_floor_div(high, cross) == INT32_MAX &&
	     sa_ag_rule<SA_AGGLO_AVERAGE>::score(low, cross) == INT32_MIN && sa_ag_rule<SA_AGGLO_AVERAGE>::combine(low / 2, low / 2) == low;
	if (!ok) {
		printf("index arithmetic wrong at N = 131072\n");
		return 1;
	}
	printf("index ok\n");
	return 0;
}

struct Case {
	int32_t num;
	std::vector<int32_t> packed; /* (exactly as long as the packed matrix: ASan sees any index beyond it) */
};

static Case make_case(uint64_t seed, int32_t num, int32_t spread)
{
	Case c;
	c.num = num;
	std::mt19937_64 rng(seed);
	c.packed.resize((size_t)num * (num - 1) / 2);
	for (int32_t &v : c.packed)
		v = (int32_t)(rng() % (uint64_t)spread) - spread / 2;
	if (spread >= 1000 && num >= 16) { /* the edge values among them */
		c.packed[0] = INT32_MAX;
		c.packed[c.packed.size() / 2] = INT32_MIN;
		c.packed[c.packed.size() - 1] = INT32_MIN;
	}
	return c;
}

/* the restatement from the members: nothing is carried from step to step but who is in which cluster */
template <int M> static void tree_from_members(const Case &cs, std::vector<int32_t> &pairs, std::vector<int32_t> &score)
{
	const int32_t num = cs.num;
	std::vector<std::vector<int32_t>> members((size_t)num);
	for (int32_t v = 0; v < num; v++)
		members[(size_t)v] = { v };
	for (int32_t t = 0; t + 1 < num; t++) {
		int32_t ba = -1, bb = -1;
		i128 bs = 0;
		int64_t bn = 1;
		for (int32_t b = 1; b < num; b++)
			for (int32_t a = 0; a < b; a++) {
				if (members[(size_t)a].empty() || members[(size_t)b].empty())
					continue;
				i128 s = M == SA_AGGLO_COMPLETE ? (i128)INT32_MAX : 0;
				for (int32_t x : members[(size_t)a])
					for (int32_t y : members[(size_t)b]) {
						const int32_t v = cs.packed[(size_t)sa_lk_packed_at(x, y)];
						s = M == SA_AGGLO_COMPLETE ? std::min(s, (i128)v) : s + v;
					}
				const int64_t n = M == SA_AGGLO_COMPLETE ? 1 : (int64_t)(members[(size_t)a].size() * members[(size_t)b].size());
				const int c = ba < 0 ? 1 : sign(s * bn - bs * n);
				if (c > 0 || (c == 0 && sa_lk_packed_at(a, b) < sa_lk_packed_at(ba, bb))) {
					ba = a, bb = b, bs = s, bn = n;
				}
			}
		pairs[2 * (size_t)t] = ba;
		pairs[2 * (size_t)t + 1] = bb;
		i128 q = bs / bn;
		if (bs % bn != 0 && bs < 0)
			q--;
		score[(size_t)t] = (int32_t)q;
		members[(size_t)ba].insert(members[(size_t)ba].end(), members[(size_t)bb].begin(), members[(size_t)bb].end());
		members[(size_t)bb].clear();
	}
}

/* the device's steps (csrc/sa_agglo.hip) with the same core functions */
template <int M> struct Replay {
	typedef typename sa_ag_rule<M>::T T;
	int32_t num;
	std::vector<T> w, bsim;
	std::vector<int32_t> size, active, best;
	int64_t rescans = 0;

	struct Cand {
		T s = 0;
		int64_t n = 1, p = 0;
		bool h = false;
		void take_if_first(const Cand &o)
		{
			if (o.h && (!h || sa_ag_before<M>(o.s, o.n, o.p, s, n, p)))
				*this = o;
		}
	};

	/* scan of row c: 64 lanes stride the row, a later equal similarity never replaces; then the reduction */
	Cand scan_row(int32_t c) const
	{
		Cand lanes[64];
		for (int lane = 0; lane < 64; lane++) {
			int32_t at = 0;
			for (int32_t d = lane; d < num; d += 64)
				if (d != c && active[(size_t)d]) {
					const T v = w[(size_t)sa_ag_at(c, d, num)];
					const int64_t n = size[(size_t)d];
					if (!lanes[lane].h || sa_ag_rule<M>::cmp(v, n, lanes[lane].s, lanes[lane].n) > 0) {
						lanes[lane].h = true, lanes[lane].s = v, lanes[lane].n = n;
						at = d;
					}
				}
			lanes[lane].p = lanes[lane].h ? sa_lk_packed_at(c, at) : 0;
		}
		for (int d = 32; d >= 1; d >>= 1) { /* the butterfly: every lane ends with the wave's first */
			Cand next[64];
			for (int lane = 0; lane < 64; lane++) {
				next[lane] = lanes[lane];
				next[lane].take_if_first(lanes[lane ^ d]);
			}
			std::copy(next, next + 64, lanes);
		}
		for (int lane = 1; lane < 64; lane++)
			if (lanes[lane].h != lanes[0].h || lanes[lane].p != lanes[0].p || lanes[lane].s != lanes[0].s) {
				printf("the lanes disagree after the reduction\n");
				exit(1);
			}
		return lanes[0];
	}

	static int32_t partner(int64_t p, int32_t c)
	{
		int64_t lo, hi;
		sa_lk_unpack(p, &lo, &hi);
		return (int32_t)(lo == c ? hi : lo);
	}

	void store_best(int32_t c, const Cand &first)
	{
		best[(size_t)c] = first.h ? partner(first.p, c) : -1;
		bsim[(size_t)c] = first.s;
	}

	int run(const Case &cs, std::vector<int32_t> &pairs, std::vector<int32_t> &score)
	{
		num = cs.num;
		const size_t n = (size_t)num;
		w.assign(n * n, 0), bsim.assign(n, 0), size.assign(n, 1), active.assign(n, 1), best.assign(n, -1);
		for (int32_t r = 0; r < num; r++) /* expand */
			for (int32_t c = 0; c < num; c++)
				if (r != c)
					w[(size_t)sa_ag_at(r, c, num)] = cs.packed[(size_t)sa_lk_packed_at(r, c)];
		for (int32_t c = 0; c < num; c++) /* scan */
			store_best(c, scan_row(c));
		for (int32_t t = 0; t + 1 < num; t++) {
			/* pick */
			Cand first;
			for (int32_t c = 0; c < num; c++) {
				if (!active[(size_t)c])
					continue;
				const int32_t d = best[(size_t)c];
				if (d < 0 || d >= num || d == c || !active[(size_t)d]) {
					printf("step %d: row %d caches partner %d\n", t, c, d);
					return 1;
				}
				Cand o;
				o.h = true, o.s = bsim[(size_t)c], o.n = (int64_t)size[(size_t)c] * size[(size_t)d], o.p = sa_lk_packed_at(c, d);
				if (o.s != w[(size_t)sa_ag_at(c, d, num)]) {
					printf("step %d: row %d caches a similarity that is not its entry\n", t, c);
					return 1;
				}
				first.take_if_first(o);
			}
			int64_t lo, hi;
			sa_lk_unpack(first.p, &lo, &hi);
			const int32_t a = (int32_t)lo, b = (int32_t)hi;
			pairs[2 * (size_t)t] = a;
			pairs[2 * (size_t)t + 1] = b;
			score[(size_t)t] = sa_ag_rule<M>::score(first.s, first.n);
			size[(size_t)a] += size[(size_t)b];
			active[(size_t)b] = 0;
			/* merge: the other rows first, from row a as it was -- on the device they never read it */
			std::vector<T> row_a(n);
			for (int32_t d = 0; d < num; d++)
				row_a[(size_t)d] = w[(size_t)sa_ag_at(a, d, num)];
			for (int32_t c = 0; c < num; c++) {
				if (c == a || !active[(size_t)c])
					continue;
				const T v = sa_ag_rule<M>::combine(w[(size_t)sa_ag_at(c, a, num)], w[(size_t)sa_ag_at(c, b, num)]);
				const int32_t old = best[(size_t)c];
				const int what = sa_ag_cache<M>(c, a, b, old, bsim[(size_t)c], sa_ag_size_before(size.data(), old, a, b), v, size[(size_t)a]);
				w[(size_t)sa_ag_at(c, a, num)] = v;
				if (what == SA_AG_RESCAN) {
					store_best(c, scan_row(c));
					rescans++;
				} else if (what == SA_AG_TAKE) {
					best[(size_t)c] = a;
					bsim[(size_t)c] = v;
				}
			}
			for (int32_t d = 0; d < num; d++)
				if (d != a && active[(size_t)d])
					w[(size_t)sa_ag_at(a, d, num)] = sa_ag_rule<M>::combine(row_a[(size_t)d], w[(size_t)sa_ag_at(b, d, num)]);
			store_best(a, scan_row(a));
			/* every cache is the first of its row again */
			for (int32_t c = 0; c < num; c++) {
				if (!active[(size_t)c] || t + 2 == num)
					continue;
				const Cand again = scan_row(c);
				if (!again.h || partner(again.p, c) != best[(size_t)c] || again.s != bsim[(size_t)c]) {
					printf("step %d: the cache of row %d is not the first of the row\n", t, c);
					return 1;
				}
			}
		}
		return 0;
	}
};

template <int M> static int replay_check(const Case &cs, int32_t spread)
{
	const size_t merges = (size_t)cs.num - 1;
	std::vector<int32_t> want_p(2 * merges), want_s(merges), got_p(2 * merges), got_s(merges);
	if (sa_ag_tree_serial<M>(cs.packed.data(), cs.num, want_p.data(), want_s.data())) {
		printf("no memory\n");
		return 1;
	}
	if (cs.num <= 65) {
		std::vector<int32_t> p(2 * merges), s(merges);
		tree_from_members<M>(cs, p, s);
		if (p != want_p || s != want_s) {
			printf("the serial tree is not the restatement from the members\n");
			return 1;
		}
	}
	Replay<M> replay;
	if (replay.run(cs, got_p, got_s))
		return 1;
	if (got_p != want_p || got_s != want_s) {
		printf("the replay of the device's steps is not the serial tree\n");
		return 1;
	}
	std::vector<int32_t> up((size_t)cs.num);
	if (sa_lk_check(got_p.data(), nullptr, cs.num, up.data()) != SA_LK_OK) {
		printf("not a tree\n");
		return 1;
	}
	for (size_t t = 1; t < merges; t++)
		if (got_s[t] > got_s[t - 1]) {
			printf("score increases at merge %zu\n", t);
			return 1;
		}
	if (spread == 1)
		for (size_t t = 0; t < merges; t++)
			if (got_p[2 * t] != 0 || got_p[2 * t + 1] != (int32_t)t + 1) {
				printf("all equal: merge %zu is not (0, %zu)\n", t, t + 1);
				return 1;
			}
	printf("replay ok: %d rows, %zu merges, %lld rescans\n", cs.num, merges, (long long)replay.rescans);
	return 0;
}

template <int M> static int cut_check(const Case &cs)
{
	const int32_t num = cs.num;
	const size_t merges = (size_t)num - 1;
	std::vector<int32_t> pairs(2 * merges), score(merges), labels((size_t)num), want((size_t)num);
	if (sa_ag_tree_serial<M>(cs.packed.data(), num, pairs.data(), score.data()))
		return 1;
	const int32_t lowest = score[merges - 1], highest = score[0];
	const int32_t cuts[7] = { lowest == INT32_MIN ? lowest : lowest - 1, lowest, score[merges / 2], highest, highest == INT32_MAX ? highest : highest + 1,
				  INT32_MIN, INT32_MAX };
	for (int32_t t : cuts) {
		/* the double loop: relabel the larger name of every merged pair, merge by merge */
		for (int32_t v = 0; v < num; v++)
			want[(size_t)v] = v;
		int32_t clusters = num;
		for (size_t m = 0; m < merges && score[m] >= t; m++) {
			const int32_t a = want[(size_t)pairs[2 * m]], b = want[(size_t)pairs[2 * m + 1]];
			for (int32_t v = 0; v < num; v++)
				if (want[(size_t)v] == std::max(a, b))
					want[(size_t)v] = std::min(a, b);
			clusters--;
		}
		const int32_t got = sa_ag_labels(pairs.data(), score.data(), num, t, labels.data());
		if (got != clusters || labels != want) {
			printf("labels at %d: %d clusters, want %d\n", t, got, clusters);
			return 1;
		}
		if (M == SA_AGGLO_COMPLETE) /* the promise: every pair inside a cluster scores at least t */
			for (int32_t j = 1; j < num; j++)
				for (int32_t i = 0; i < j; i++)
					if (labels[(size_t)i] == labels[(size_t)j] && cs.packed[(size_t)sa_lk_packed_at(i, j)] < t) {
						printf("complete linkage at %d: pair (%d, %d) inside a cluster scores below it\n", t, i, j);
						return 1;
					}
	}
	printf("cut ok: %d rows, 7 thresholds, %zu merges\n", num, merges);
	return 0;
}

static int refuse_check()
{
	const int32_t n = 5, poison = -0x5A5A5A5B;
	const int32_t good_p[8] = { 2, 3, 0, 1, 0, 2, 0, 4 }, good_s[4] = { 9, 9, 4, -3 }; /* (equal scores, descending p: fine here) */
	struct Bad {
		int32_t pairs[8], score[4];
		int want;
	} bad[] = {
		{ { 0, 1, 1, 2, 0, 2, 3, 4 }, { 9, 8, 7, 6 }, SA_LK_CYCLE },
		{ { 1, 0, 2, 3, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_LO_HI },
		{ { 0, 1, 2, 2, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_LO_HI },
		{ { 0, 1, 2, 3, 1, 2, 3, 5 }, { 9, 9, 4, -3 }, SA_LK_RANGE },
		{ { 0, 1, -1, 3, 1, 2, 3, 4 }, { 9, 9, 4, -3 }, SA_LK_RANGE },
		{ { 2, 3, 0, 1, 0, 2, 0, 4 }, { 9, 9, 4, 5 }, SA_AG_NOT_DESCENDING },
		{ { 2, 3, 0, 1, 0, 2, 0, 4 }, { INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN + 1 }, SA_AG_NOT_DESCENDING },
	};
	int32_t labels[5];
	for (const Bad &b : bad) {
		std::fill(labels, labels + n, poison);
		const int32_t got = sa_ag_labels(b.pairs, b.score, n, 0, labels);
		if (got != b.want || std::count(labels, labels + n, poison) != n) {
			printf("a bad tree gave %d, want %d (or labels were written)\n", got, b.want);
			return 1;
		}
	}
	if (sa_ag_labels(good_p, good_s, n, 5, labels) != 3 || labels[0] != 0 || labels[1] != 0 || labels[2] != 2 || labels[3] != 2 || labels[4] != 4) {
		printf("the good tree is refused or mislabelled\n");
		return 1;
	}
	int32_t up[5];
	if (sa_lk_check(good_p, good_s, n, up) != SA_LK_ORDER) { /* (what sa_linkage_labels rightly says of it) */
		printf("the single-linkage check accepts equal scores in descending p\n");
		return 1;
	}
	printf("refuse ok: %zu trees\n", sizeof(bad) / sizeof(bad[0]));
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--predicate"))
		return predicate_check();
	if (argc == 2 && !strcmp(argv[1], "--index"))
		return index_check();
	if (argc == 2 && !strcmp(argv[1], "--refuse"))
		return refuse_check();
	if (argc == 6 && (!strcmp(argv[1], "--replay") || !strcmp(argv[1], "--cut"))) {
		const int32_t spread = atoi(argv[4]), method = atoi(argv[5]);
		const Case cs = make_case(strtoull(argv[2], nullptr, 10), atoi(argv[3]), spread);
		if (cs.num < 2 || spread < 1 || (method != SA_AGGLO_COMPLETE && method != SA_AGGLO_AVERAGE))
			return 2;
		if (!strcmp(argv[1], "--replay"))
			return method == SA_AGGLO_COMPLETE ? replay_check<SA_AGGLO_COMPLETE>(cs, spread) : replay_check<SA_AGGLO_AVERAGE>(cs, spread);
		return method == SA_AGGLO_COMPLETE ? cut_check<SA_AGGLO_COMPLETE>(cs) : cut_check<SA_AGGLO_AVERAGE>(cs);
	}
	fprintf(stderr, "usage: agglo_test --predicate | --index | --refuse | --replay SEED N SPREAD METHOD | --cut SEED N SPREAD METHOD\n");
	return 2;
}
