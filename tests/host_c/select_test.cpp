/* select_test.cpp -- the contract of the order statistics (sequencealigner_amd/csrc/sa_select_core.h) on the host, built with
 * -fsanitize=address,undefined by tests/test_select_core.py.
 *
 *   select_test --keys                 the key transform, the byte of a round, the upper bits and the scratch layout
 *   select_test --select SEED P SPREAD P entries drawn from SPREAD (equal | pm | extremes | band | uniform): the serial count,
 *                                      narrow and regroup of the core for the rank sets {0}, {P - 1}, {P / 2}, sixteen equal
 *                                      ranks and sixteen spread ranks against std::sort: value = sorted[rank], below = the first
 *                                      place of that value; the groups of a round never exceed the ranks
 *   select_test --rank P Q WANT ...    sa_sel_rank(P, Q) against the WANT the caller computed, any number of triples
 */
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_select_core.h"

static int keys_check()
{
	const int32_t scores[] = { INT32_MIN, INT32_MIN + 1, -65536, -257, -256, -1, 0, 1, 255, 256, 65535, INT32_MAX - 1, INT32_MAX };
	const size_t n = sizeof(scores) / sizeof(scores[0]);
	for (size_t a = 0; a < n; a++) {
		const uint32_t key = sa_sel_key(scores[a]);
		if (sa_sel_score(key) != scores[a]) {
			printf("key of %d does not turn back\n", scores[a]);
			return 1;
		}
		if (a && !(sa_sel_key(scores[a - 1]) < key)) {
			printf("keys of %d and %d are not in order\n", scores[a - 1], scores[a]);
			return 1;
		}
		uint32_t again = 0;
		for (int round = 0; round < SA_SEL_ROUNDS; round++) {
			if (sa_sel_upper(key, round) != (round ? again : 0u) || sa_sel_upper(key, round) == SA_SEL_NO_UPPER ||
			    !sa_sel_shares(key, again << (round ? 32 - 8 * round : 0), round)) {
				printf("upper bits of %d in round %d\n", scores[a], round);
				return 1;
			}
			again = (again << 8) | sa_sel_byte(key, round);
		}
		if (again != key) {
			printf("the four bytes of %d do not make its key\n", scores[a]);
			return 1;
		}
	}
	if (sa_sel_key(INT32_MIN) != 0u || sa_sel_key(INT32_MAX) != 0xFFFFFFFFu || sa_sel_shares(0x12345678u, 0x12355678u, 2) ||
	    !sa_sel_shares(0x12345678u, 0x1234FFFFu, 2) || !sa_sel_shares(0u, 0xFFFFFFFFu, 0)) {
		printf("key ends or sharing wrong\n");
		return 1;
	}
	if (sa_sel_scratch_bytes(0) != 0 || sa_sel_scratch_bytes(SA_SEL_MAX + 1) != 0 || sa_sel_scratch_bytes(-1) != 0 ||
	    sa_sel_table_offset() % 8 != 0 || sa_sel_scratch_bytes(1) != sa_sel_table_offset() + 2048 ||
	    sa_sel_scratch_bytes(16) != sa_sel_table_offset() + 32768) {
		printf("scratch layout wrong\n");
		return 1;
	}
	printf("keys ok\n");
	return 0;
}

static int select(unsigned seed, int64_t pairs, const char *spread)
{
	if (pairs < 1) {
		printf("bad arguments\n");
		return 2;
	}
	std::mt19937 rng(seed);
	std::vector<int32_t> packed((size_t)pairs); /* (exactly P entries: ASan sees any index beyond them) */
	const int32_t band_at = (int32_t)(rng() % 2000000u) - 1000000;
	for (int32_t &v : packed) {
		if (!strcmp(spread, "equal"))
			v = band_at;
		else if (!strcmp(spread, "pm"))
			v = (rng() & 1u) ? 0 : -1;
		else if (!strcmp(spread, "extremes"))
			v = (rng() & 1u) ? INT32_MAX : INT32_MIN;
		else if (!strcmp(spread, "band"))
			v = band_at + (int32_t)(rng() % 300u);
		else if (!strcmp(spread, "uniform"))
			v = (int32_t)(uint32_t)rng();
		else {
			printf("unknown spread %s\n", spread);
			return 2;
		}
	}
	std::vector<int32_t> sorted(packed);
	std::sort(sorted.begin(), sorted.end());
	std::vector<std::vector<int64_t>> sets = { { 0 }, { pairs - 1 }, { pairs / 2 }, {}, {} };
	for (int i = 0; i < SA_SEL_MAX; i++) {
		sets[3].push_back(pairs / 2);
		sets[4].push_back((int64_t)((15 - i) * pairs / 16)); /* (descending: the caller's order is no sorted order) */
	}
	int32_t most = 0;
	for (const std::vector<int64_t> &ranks : sets) {
		const int32_t m = (int32_t)ranks.size();
		std::vector<int32_t> value((size_t)m, 12345);
		std::vector<int64_t> below((size_t)m, -7);
		std::vector<uint64_t> table((size_t)m * SA_SEL_BINS, ~(uint64_t)0); /* (exactly m groups of bins, contents ignored) */
		sa_sel_state st;
		memset(&st, 0xFF, sizeof(st));
		int32_t groups = 0;
		sa_sel_serial(packed.data(), pairs, ranks.data(), m, value.data(), below.data(), &st, table.data(), &groups);
		if (groups < 1 || groups > m) {
			printf("%d groups for %d ranks\n", groups, m);
			return 1;
		}
		most = std::max(most, groups);
		for (int32_t t = 0; t < m; t++) {
			const int32_t want = sorted[(size_t)ranks[(size_t)t]];
			const int64_t first = std::lower_bound(sorted.begin(), sorted.end(), want) - sorted.begin();
			if (value[(size_t)t] != want || below[(size_t)t] != first) {
				printf("rank %lld of %lld (%s): value %d below %lld, sorted says %d and %lld\n", (long long)ranks[(size_t)t],
				       (long long)pairs, spread, value[(size_t)t], (long long)below[(size_t)t], want, (long long)first);
				return 1;
			}
		}
	}
	printf("select ok: %lld entries, %zu rank sets, %d groups at most\n", (long long)pairs, sets.size(), most);
	return 0;
}

static int rank_table(int count, char **args)
{
	for (int k = 0; k + 2 < count; k += 3) {
		const int64_t pairs = strtoll(args[k], nullptr, 10), want = strtoll(args[k + 2], nullptr, 10);
		const double q = strtod(args[k + 1], nullptr);
		const int64_t got = sa_sel_rank(pairs, q);
		if (got != want) {
			printf("sa_sel_rank(%lld, %s) = %lld, the caller says %lld\n", (long long)pairs, args[k + 1], (long long)got, (long long)want);
			return 1;
		}
	}
	printf("rank ok: %d cases\n", count / 3);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--keys"))
		return keys_check();
	if (argc == 5 && !strcmp(argv[1], "--select"))
		return select((unsigned)atoi(argv[2]), strtoll(argv[3], nullptr, 10), argv[4]);
	if (argc >= 5 && (argc - 2) % 3 == 0 && !strcmp(argv[1], "--rank"))
		return rank_table(argc - 2, argv + 2);
	printf("usage: select_test --keys | --select SEED P SPREAD | --rank P Q WANT ...\n");
	return 2;
}
