/* neighbors_test.cpp -- the ordering contract of the nearest-neighbour selection (sequencealigner_amd/csrc/sa_neighbors_core.h)
 * on the host, built with -fsanitize=address,undefined by tests/test_neighbors_core.py.
 *
 *   neighbors_test --keys            key order == (score descending, index ascending) over the extreme scores and indices
 *   neighbors_test --rows SEED N K SPREAD
 *                                    a random symmetric matrix of N sequences whose scores take SPREAD distinct values (heavy
 *                                    ties for a small SPREAD): sa_nb_select_row of every row against std::partial_sort with
 *                                    the contract's comparator
 */
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/seqalign_hip.h"
#include "../../sequencealigner_amd/csrc/sa_neighbors_core.h"

struct Cand {
	int32_t score, index;
};
/* the contract, spelled out: better first */
static bool better(const Cand &a, const Cand &b) { return a.score != b.score ? a.score > b.score : a.index < b.index; }

static int keys()
{
	const int32_t scores[] = { INT32_MIN, INT32_MIN + 1, SA_SCORE_MIN, SA_SCORE_MIN + 1, -1000, -1, 0, 1, 1000, INT32_MAX - 1, INT32_MAX };
	const int32_t indices[] = { 0, 1, 2, 63, 64, 65, 89999, INT32_MAX - 1, INT32_MAX };
	std::vector<Cand> all;
	for (int32_t s : scores)
		for (int32_t c : indices)
			all.push_back({ s, c });
	for (const Cand &a : all) {
		const uint64_t ka = sa_nb_key(a.score, a.index);
		if (sa_nb_key_score(ka) != a.score || sa_nb_key_index(ka) != a.index) {
			printf("key of (%d, %d) does not decode\n", a.score, a.index);
			return 1;
		}
		if (!(ka > SA_NB_EMPTY)) {
			printf("key of (%d, %d) is not above the empty entry\n", a.score, a.index);
			return 1;
		}
		for (const Cand &b : all) {
			const uint64_t kb = sa_nb_key(b.score, b.index);
			if ((ka > kb) != better(a, b) || (ka == kb) != (a.score == b.score && a.index == b.index)) {
				printf("key order of (%d, %d) against (%d, %d) differs from the contract\n", a.score, a.index, b.score, b.index);
				return 1;
			}
		}
	}
	/* the packed index of both triangles */
	if (sa_nb_packed_at(0, 1) != 0 || sa_nb_packed_at(1, 0) != 0 || sa_nb_packed_at(2, 1) != 2 || sa_nb_packed_at(3, 0) != 3 ||
	    sa_nb_packed_at(0, 89999) != (int64_t)89999 * 89998 / 2 || sa_nb_packed_at(89999, 89998) != (int64_t)89999 * 89998 / 2 + 89998) {
		printf("packed index wrong\n");
		return 1;
	}
	printf("keys ok: %zu candidates\n", all.size());
	return 0;
}

static int rows(unsigned seed, int32_t num, int32_t k, int32_t spread)
{
	if (num < 2 || k < 1 || k > SA_HIP_NEIGHBORS_MAX || k > num - 1 || spread < 1) {
		printf("bad arguments\n");
		return 2;
	}
	std::mt19937 rng(seed);
	const size_t pairs = (size_t)num * (size_t)(num - 1) / 2;
	std::vector<int32_t> packed(pairs); /* (exactly as long as the packed matrix: ASan sees any index beyond it) */
	for (int32_t &v : packed) {
		v = (int32_t)(rng() % (uint32_t)spread) - spread / 2;
		if (rng() % 97 == 0) /* a few extremes among them */
			v = rng() % 2 ? INT32_MIN : INT32_MAX;
	}
	std::vector<int32_t> index((size_t)k), score((size_t)k);
	std::vector<Cand> cands;
	size_t tied_rows = 0;
	for (int32_t r = 0; r < num; r++) {
		sa_nb_select_row(packed.data(), num, r, k, index.data(), score.data());
		cands.clear();
		for (int32_t c = 0; c < num; c++)
			if (c != r)
				cands.push_back({ packed[(size_t)sa_nb_packed_at(r, c)], c });
		std::partial_sort(cands.begin(), cands.begin() + k, cands.end(), better);
		for (int32_t t = 0; t < k; t++)
			if (index[(size_t)t] != cands[(size_t)t].index || score[(size_t)t] != cands[(size_t)t].score) {
				printf("row %d entry %d: got (%d, %d), partial_sort says (%d, %d)\n", r, t, score[(size_t)t], index[(size_t)t],
				       cands[(size_t)t].score, cands[(size_t)t].index);
				return 1;
			}
		if ((size_t)k < cands.size()) {
			std::nth_element(cands.begin() + k, cands.begin() + k, cands.end(), better);
			tied_rows += cands[(size_t)k].score == cands[(size_t)k - 1].score;
		}
	}
	printf("rows ok: %d rows, k = %d, %zu rows with a tie across the cut\n", num, k, tied_rows);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--keys"))
		return keys();
	if (argc == 6 && !strcmp(argv[1], "--rows"))
		return rows((unsigned)atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
	printf("usage: neighbors_test --keys | --rows SEED N K SPREAD\n");
	return 2;
}
