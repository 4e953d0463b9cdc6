/* search_above_test.cpp -- the host-compilable core of the threshold search (csrc/sa_search_above_core.h) against a plain loop.
 * Built by tests/test_search_above_core.py with g++ -fsanitize=address,undefined; every buffer is a heap array of exactly the
 * size the contract gives it, so a write past a row's end or past the scratch is an ASan report.
 *
 *   --rule              the segment rule at its edges and the scratch size
 *   --csr N S           count / scan / fill of 4 rows of N candidates cut into S segments, for every kind of content and
 *                       every threshold (below, inside and above the values, INT32_MIN, INT32_MAX), with and without value /
 *                       score, score from another rectangle and from the same
 */
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_search_above_core.h"

#define CHECK(cond, ...)                                   \
	do {                                               \
		if (!(cond)) {                             \
			fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
			fprintf(stderr, __VA_ARGS__);      \
			fprintf(stderr, "\n");             \
			exit(1);                           \
		}                                          \
	} while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 32);
}

static int rule()
{
	/* the rows alone fill the device */
	CHECK(sa_above_segments(1000000, SA_HITS_ROWS_FILL) == 1, "S at ROWS_FILL");
	CHECK(sa_above_segments(1000000, SA_HITS_ROWS_FILL - 1) == (SA_HITS_WAVES + SA_HITS_ROWS_FILL - 2) / (SA_HITS_ROWS_FILL - 1), "S below ROWS_FILL");
	CHECK(sa_above_segments(INT32_MAX, INT32_MAX) == 1, "S at the largest shape");
	/* held to N / 64: a segment is at least one step long */
	CHECK(sa_above_segments(1, 1) == 1 && sa_above_segments(63, 1) == 1 && sa_above_segments(64, 1) == 1, "short rows");
	CHECK(sa_above_segments(65, 3) == 1 && sa_above_segments(127, 3) == 1, "one step and a tail");
	CHECK(sa_above_segments(128, 4) == 2 && sa_above_segments(130, 4) == 2, "two segments");
	CHECK(sa_hits_seg_begin(130, 2, 1) == 65, "the cut of (4, 130)");
	CHECK(sa_above_segments(200003, 2) == 3125, "N / 64 segments");
	CHECK(sa_above_segments(70, 3000) == 1, "many rows");
	/* about SA_HITS_WAVES waves when the rows are long */
	CHECK(sa_above_segments(INT32_MAX, 1) == SA_HITS_WAVES, "one long row");
	CHECK(sa_above_segments(1000000, 3) == (SA_HITS_WAVES + 2) / 3, "three long rows");
	for (int32_t nq : { 1, 2, 3, 7, 100, 2047, 2048, 5000 })
		for (int32_t n : { 1, 63, 64, 65, 127, 128, 1000, 4096, 200003, 1 << 20, INT32_MAX }) {
			const int32_t S = sa_above_segments(n, nq);
			CHECK(S >= 1, "S >= 1");
			CHECK((int64_t)nq * S < SA_HITS_WAVES + (int64_t)nq || S == 1, "waves (%d, %d)", n, nq);
			if (S > 1)
				for (int32_t s : { 0, 1, S / 2, S - 1 }) /* every segment at least one step long */
					CHECK(sa_hits_seg_begin(n, S, s + 1) - sa_hits_seg_begin(n, S, s) >= SA_ABOVE_STEP, "segment %d of %d over %d", s, S, n);
			CHECK(sa_hits_seg_begin(n, S, 0) == 0 && sa_hits_seg_begin(n, S, S) == n, "cover");
			CHECK(sa_above_scratch_elems(n, nq) == (int64_t)nq * S + 1, "scratch");
		}
	printf("rule ok\n");
	return 0;
}

enum Kind { THREE, EQUAL, RANDOM, EXTREME };

static void make(std::vector<int32_t> &a, Kind kind)
{
	for (auto &x : a) {
		switch (kind) {
		case THREE:
			x = (int32_t)(rng() % 3) - 1;
			break;
		case EQUAL:
			x = 7;
			break;
		case RANDOM:
			x = (int32_t)(rng() % 2001) - 1000;
			break;
		default:
			x = (rng() & 1) ? INT32_MAX : (rng() & 1) ? INT32_MIN : (int32_t)rng();
			break;
		}
	}
}

static int csr(int32_t n, int32_t S)
{
	const int32_t nq = 4;
	int64_t combos = 0, hits_total = 0;
	for (Kind kind : { THREE, EQUAL, RANDOM, EXTREME }) {
		std::vector<int32_t> vrect((size_t)nq * n), rect((size_t)nq * n);
		make(vrect, kind);
		make(rect, RANDOM);
		for (int32_t t : { INT32_MIN, -1001, -1, 0, 1, 7, 8, 500, 1001, INT32_MAX - 1, INT32_MAX }) {
			/* the expectation: a plain loop */
			std::vector<int64_t> want_off(nq + 1, 0);
			std::vector<int32_t> want_idx, want_val, want_sco;
			for (int32_t r = 0; r < nq; r++) {
				for (int32_t d = 0; d < n; d++)
					if (vrect[(size_t)r * n + d] >= t) {
						want_idx.push_back(d);
						want_val.push_back(vrect[(size_t)r * n + d]);
						want_sco.push_back(rect[(size_t)r * n + d]);
					}
				want_off[r + 1] = (int64_t)want_idx.size();
			}
			const size_t e = want_idx.size();
			/* count, scan, offsets: exact-size heap arrays */
			int64_t *scratch = new int64_t[(size_t)nq * S + 1];
			int64_t *offsets = new int64_t[nq + 1];
			for (int32_t r = 0; r < nq; r++)
				sa_above_count_row(vrect.data() + (size_t)r * n, n, S, t, scratch + (size_t)r * S);
			sa_above_scan(scratch, (int64_t)nq * S);
			sa_above_offsets(scratch, nq, S, offsets);
			CHECK(memcmp(offsets, want_off.data(), sizeof(int64_t) * (nq + 1)) == 0, "offsets N=%d S=%d t=%d", n, S, t);
			CHECK(scratch[(size_t)nq * S] == (int64_t)e, "total");
			for (int variant = 0; variant < 3; variant++) { /* another rectangle; the same; no value / score */
				int32_t *index = new int32_t[e], *value = variant == 2 ? nullptr : new int32_t[e], *score = variant == 2 ? nullptr : new int32_t[e];
				const std::vector<int32_t> &src = variant == 0 ? rect : vrect;
				for (int32_t r = 0; r < nq; r++)
					sa_above_fill_row(vrect.data() + (size_t)r * n, score ? src.data() + (size_t)r * n : nullptr, n, S, t, scratch + (size_t)r * S,
							  offsets[r + 1], index, value, score);
				CHECK(e == 0 || memcmp(index, want_idx.data(), 4 * e) == 0, "index N=%d S=%d t=%d", n, S, t);
				if (value)
					CHECK(e == 0 || memcmp(value, want_val.data(), 4 * e) == 0, "value N=%d S=%d t=%d", n, S, t);
				if (score)
					CHECK(e == 0 || memcmp(score, (variant == 0 ? want_sco : want_val).data(), 4 * e) == 0, "score N=%d S=%d t=%d", n, S, t);
				delete[] index;
				delete[] value;
				delete[] score;
			}
			/* the guard: with every row's end pulled in by one, nothing is written at or beyond it */
			if (e) {
				int32_t *index = new int32_t[e];
				memset(index, 0xA5, 4 * e);
				for (int32_t r = 0; r < nq; r++)
					sa_above_fill_row(vrect.data() + (size_t)r * n, nullptr, n, S, t, scratch + (size_t)r * S,
							  offsets[r + 1] > offsets[r] ? offsets[r + 1] - 1 : offsets[r + 1], index, nullptr, nullptr);
				for (int32_t r = 0; r < nq; r++)
					if (offsets[r + 1] > offsets[r])
						CHECK((uint32_t)index[offsets[r + 1] - 1] == 0xA5A5A5A5u, "guard row %d", r);
				delete[] index;
			}
			delete[] scratch;
			delete[] offsets;
			combos++;
			hits_total += (int64_t)e;
			if (t == INT32_MIN)
				CHECK(e == (size_t)nq * n, "INT32_MIN keeps everything");
			if (kind != EXTREME && t >= 1001)
				CHECK(e == 0, "above the maximum keeps nothing");
		}
	}
	printf("csr ok: N = %d, S = %d, %lld combinations, %lld hits\n", n, S, (long long)combos, (long long)hits_total);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "--rule")
		return rule();
	if (mode == "--csr" && argc == 4)
		return csr(atoi(argv[2]), atoi(argv[3]));
	fprintf(stderr, "usage: %s --rule | --csr N S\n", argv[0]);
	return 2;
}
