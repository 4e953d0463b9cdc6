/* tests/host_c/normalize_test.cpp -- the contract of the normalised scores (sequencealigner_amd/csrc/sa_normalize_core.h) on the
 * host, under ASan / UBSan (tests/test_normalize_core.py builds and runs it).  The expectation is __int128 arithmetic with an
 * explicit floor, never the code's own double quotient.
 *   --grid               sa_norm_value_rule over the grid of edge values, all three rules
 *   --random SEED COUNT  ... over COUNT random triples
 *   --triangle N SEED    the serial whole-triangle walk (the kernel's deal of columns) against the direct formula per (i, j)
 *   --index N            the index functions at N: every column once, starts in order, the last entry at P - 1 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_normalize_core.h"

static const int64_t PPM = 1000000;

/* the contract, in 128 bits */
static int32_t expect(int32_t s, int32_t di, int32_t dj, int rule)
{
	__int128 den, num = (__int128)s * PPM;
	if (rule == 0)
		den = di < dj ? di : dj;
	else if (rule == 1)
		den = di > dj ? di : dj;
	else {
		den = (__int128)di + dj;
		num *= 2;
	}
	if (den <= 0)
		return INT32_MIN;
	__int128 q = num / den; /* truncates */
	if (num % den != 0 && num < 0)
		q -= 1;
	if (q < INT32_MIN)
		return INT32_MIN;
	if (q > INT32_MAX)
		return INT32_MAX;
	return (int32_t)q;
}

static long check(int32_t s, int32_t di, int32_t dj)
{
	long bad = 0;
	for (int rule = 0; rule < 3; rule++) {
		const int32_t got = sa_norm_value_rule(s, di, dj, rule), want = expect(s, di, dj, rule);
		if (got != want) {
			if (bad++ < 10)
				printf("MISMATCH rule %d: s %d di %d dj %d: got %d, want %d\n", rule, s, di, dj, got, want);
		}
	}
	return bad;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "--grid")) {
		const int32_t g[] = { INT32_MIN, INT32_MIN + 1, -1000000, -1, 0, 1, 2, 3, 999999, 1000000, 1000001, INT32_MAX - 1, INT32_MAX };
		const int n = (int)(sizeof(g) / sizeof(g[0]));
		long bad = 0, cases = 0;
		for (int a = 0; a < n; a++)
			for (int b = 0; b < n; b++)
				for (int c = 0; c < n; c++) {
					bad += check(g[a], g[b], g[c]);
					cases += 3;
				}
		/* what the floor rule means, spelled out once */
		if (sa_norm_value_rule(-1, 3, 3, SA_NORM_RULE_MIN) != -333334 || sa_norm_value_rule(1, 3, 3, SA_NORM_RULE_MIN) != 333333 ||
		    sa_norm_value_rule(-1, 3, 7, SA_NORM_RULE_MEAN) != -200000 || sa_norm_value_rule(-1, 3, 4, SA_NORM_RULE_MEAN) != -285715 ||
		    sa_norm_value_rule(5, 0, 7, SA_NORM_RULE_MIN) != INT32_MIN || sa_norm_value_rule(5, 0, 7, SA_NORM_RULE_MAX) != 714285 ||
		    sa_norm_value_rule(5, -7, 7, SA_NORM_RULE_MEAN) != INT32_MIN || sa_norm_value_rule(INT32_MAX, 1, 1, SA_NORM_RULE_MAX) != INT32_MAX ||
		    sa_norm_value_rule(INT32_MIN, 1, 1, SA_NORM_RULE_MIN) != INT32_MIN || sa_norm_value_rule(12345, 1000000, 1000000, SA_NORM_RULE_MEAN) != 12345)
			bad++;
		if (bad)
			return printf("grid FAILED: %ld mismatches\n", bad), 1;
		printf("grid ok: %ld cases\n", cases);
		return 0;
	}
	if (argc >= 4 && !strcmp(argv[1], "--random")) {
		std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
		const long count = atol(argv[3]);
		long bad = 0, negative_inexact = 0;
		for (long t = 0; t < count; t++) {
			/* a third each: anything; small denominators; large scores over large denominators (quotients near integers) */
			int32_t s = (int32_t)(uint32_t)rng(), di = (int32_t)(uint32_t)rng(), dj = (int32_t)(uint32_t)rng();
			if (t % 3 == 1) {
				di = (int32_t)(rng() % 4000) - 100;
				dj = (int32_t)(rng() % 4000) - 100;
				s = (int32_t)(rng() % 200001) - 100000;
			} else if (t % 3 == 2) {
				di = (int32_t)(rng() >> 33) | 1;
				dj = (int32_t)(rng() >> 33) | 1;
			}
			bad += check(s, di, dj);
			const int64_t d = di < dj ? di : dj;
			if (s < 0 && d > 0 && ((int64_t)s * PPM) % d != 0)
				negative_inexact++;
		}
		if (bad)
			return printf("random FAILED: %ld mismatches\n", bad), 1;
		printf("random ok: %ld triples, %ld negative inexact quotients\n", count, negative_inexact);
		return 0;
	}
	if (argc >= 4 && !strcmp(argv[1], "--triangle")) {
		const int32_t num = atoi(argv[2]);
		std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
		const int64_t pairs = (int64_t)num * (num - 1) / 2;
		std::vector<int32_t> in((size_t)pairs), den((size_t)num), out((size_t)pairs + 8, 0x5A5A5A5A);
		for (auto &v : in)
			v = (int32_t)(rng() % 4001) - 2000;
		for (auto &v : den)
			v = (int32_t)(rng() % 300) - 3; /* (a few <= 0) */
		long bad = 0;
		for (int rule = 0; rule < 3; rule++) {
			std::fill(out.begin(), out.end(), 0x5A5A5A5A);
			sa_norm_triangle(in.data(), den.data(), num, rule, out.data());
			for (int64_t j = 1; j < num; j++)
				for (int64_t i = 0; i < j; i++) {
					const int64_t p = j * (j - 1) / 2 + i;
					if (out[(size_t)p] != expect(in[(size_t)p], den[(size_t)i], den[(size_t)j], rule))
						bad++;
				}
			for (size_t k = (size_t)pairs; k < out.size(); k++)
				bad += out[k] != 0x5A5A5A5A;
			/* in place: the same bytes */
			std::vector<int32_t> same(in);
			sa_norm_triangle(same.data(), den.data(), num, rule, same.data());
			bad += memcmp(same.data(), out.data(), sizeof(int32_t) * (size_t)pairs) != 0;
		}
		if (bad)
			return printf("triangle FAILED: %ld mismatches\n", bad), 1;
		printf("triangle ok: %d sequences, %lld pairs, 3 rules\n", num, (long long)pairs);
		return 0;
	}
	if (argc >= 3 && !strcmp(argv[1], "--index")) {
		const int64_t num = atoll(argv[2]);
		const int64_t pairs = num * (num - 1) / 2;
		std::vector<uint8_t> seen((size_t)num, 0);
		long bad = 0;
		int64_t entries = 0, longest = 0, shortest = INT64_MAX;
		for (int64_t t = 0; t < sa_norm_units(num); t++) {
			int64_t a, b;
			sa_norm_deal(num, t, &a, &b);
			int64_t work = 0;
			for (int64_t j : { a, b }) {
				if (j < 0)
					continue;
				if (j >= num || seen[(size_t)j]++)
					bad++;
				if (sa_norm_column_start(j) + j != sa_norm_column_start(j + 1)) /* runs tile the packed index without gaps */
					bad++;
				work += j;
			}
			entries += work;
			longest = work > longest ? work : longest;
			shortest = work < shortest ? work : shortest;
		}
		for (int64_t j = 0; j < num; j++)
			bad += seen[(size_t)j] != 1;
		bad += entries != pairs;
		bad += sa_norm_column_start(num - 1) + (num - 1) != pairs; /* the last entry sits at P - 1 */
		bad += longest != num - 1;                                  /* every unit but a lone middle column holds N - 1 entries */
		bad += !(shortest == num - 1 || (num % 2 == 1 && shortest == (num - 1) / 2));
		if (num >= 92683)
			bad += sa_norm_column_start(num - 1) + (num - 1) <= (int64_t)UINT32_MAX; /* (P passes 2^32 here: 64-bit on purpose) */
		if (bad)
			return printf("index FAILED: %ld\n", bad), 1;
		printf("index ok: %lld columns, %lld entries, last start %lld\n", (long long)num, (long long)entries, (long long)sa_norm_column_start(num - 1));
		return 0;
	}
	printf("usage: normalize_test --grid | --random SEED COUNT | --triangle N SEED | --index N\n");
	return 2;
}
