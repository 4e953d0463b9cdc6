/* traceback_test.cpp -- the traceback contract (include/seqalign_hip.h, "alignments for chosen pairs") on the host, built with
 * -fsanitize=address,undefined by tests/test_traceback_core.py.
 *
 *   traceback_test METHOD SEED PAIRS MAXLEN ALPHABET GAP1 GAP2
 *       METHOD 0 NW (gap GAP1), 1 Gotoh, 2 SW (open GAP1, extend GAP2; given positive, stored negated).  PAIRS random pairs
 *       of lengths 1 .. MAXLEN over ALPHABET residue codes (1: homopolymers, every tie exists), each in both orders (a < b
 *       and a > b).  Per pair: the full tables are filled with the reference's recurrences (nw.c, ga.c, sw.c); every computed
 *       cell is recorded through the core's encoder at the core's scratch offset; the records are walked with the core's
 *       step and run-length emitter; the result is compared with literal(), a separate implementation of the contract that
 *       reads the full tables and nothing of the core.  The CIGAR is also re-scored by the documented rule.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/seqalign_hip.h"
#include "../../sequencealigner_amd/csrc/sa_traceback_core.h"

static const int32_t SMIN = SA_SCORE_MIN;
static int32_t S[SA_SUB_DIM][SA_SUB_DIM];

struct Tables {
	int32_t m, n;
	std::vector<int32_t> M, X, Y;
	int32_t &at(std::vector<int32_t> &t, int32_t r, int32_t c) { return t[(size_t)r * (n + 1) + c]; }
	int32_t get(const std::vector<int32_t> &t, int32_t r, int32_t c) const { return t[(size_t)r * (n + 1) + c]; }
};

/* S of cell (r, c) as the score kernels index it: NW sub[lo][hi], Gotoh / SW sub[hi][lo] */
static int32_t sim(int method, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t r, int32_t c)
{
	return method == SA_METHOD_NW ? S[lo[r - 1]][hi[c - 1]] : S[hi[c - 1]][lo[r - 1]];
}

static Tables fill(int method, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t g, int32_t o, int32_t e)
{
	Tables T;
	T.m = (int32_t)lo.size();
	T.n = (int32_t)hi.size();
	const size_t cells = (size_t)(T.m + 1) * (T.n + 1);
	T.M.assign(cells, 0);
	T.X.assign(cells, SMIN);
	T.Y.assign(cells, SMIN);
	if (method == SA_METHOD_NW) {
		for (int32_t c = 0; c <= T.n; c++)
			T.at(T.M, 0, c) = c * g;
		for (int32_t r = 0; r <= T.m; r++)
			T.at(T.M, r, 0) = r * g;
	} else if (method == SA_METHOD_GA) {
		for (int32_t c = 1; c <= T.n; c++) {
			T.at(T.X, 0, c) = std::max(T.get(T.M, 0, c - 1) + o, T.get(T.X, 0, c - 1) + e);
			T.at(T.M, 0, c) = T.get(T.X, 0, c);
		}
		for (int32_t r = 1; r <= T.m; r++) {
			T.at(T.Y, r, 0) = std::max(T.get(T.M, r - 1, 0) + o, T.get(T.Y, r - 1, 0) + e);
			T.at(T.M, r, 0) = T.get(T.Y, r, 0);
		}
	}
	for (int32_t r = 1; r <= T.m; r++)
		for (int32_t c = 1; c <= T.n; c++) {
			const int32_t sd = T.get(T.M, r - 1, c - 1) + sim(method, lo, hi, r, c);
			if (method == SA_METHOD_NW) {
				T.at(T.M, r, c) = std::max(T.get(T.M, r, c - 1) + g, std::max(T.get(T.M, r - 1, c) + g, sd));
				continue;
			}
			const int32_t x = std::max(T.get(T.M, r, c - 1) + o, T.get(T.X, r, c - 1) + e);
			const int32_t y = std::max(T.get(T.M, r - 1, c) + o, T.get(T.Y, r - 1, c) + e);
			T.at(T.X, r, c) = x;
			T.at(T.Y, r, c) = y;
			int32_t best = method == SA_METHOD_SW ? std::max(sd, 0) : sd;
			best = std::max(x, best);
			best = std::max(y, best);
			T.at(T.M, r, c) = best;
		}
	return T;
}

struct Result {
	int32_t score = 0, lo_begin = 0, lo_end = 0, hi_begin = 0, hi_end = 0, columns = 0;
	std::vector<uint32_t> runs;
	bool operator==(const Result &o) const
	{
		return score == o.score && lo_begin == o.lo_begin && lo_end == o.lo_end && hi_begin == o.hi_begin && hi_end == o.hi_end &&
		       columns == o.columns && runs == o.runs;
	}
};

/* the contract, literally, over the full tables; ops in the canonical orientation, mirrored at the end */
static Result literal(int method, const Tables &T, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t g, int32_t o,
		      bool flip)
{
	std::vector<int> ops; /* end-first */
	int32_t r = T.m, c = T.n;
	Result R;
	if (method == SA_METHOD_SW) {
		int32_t best = 0;
		for (int32_t i = 1; i <= T.m; i++)
			for (int32_t j = 1; j <= T.n; j++)
				best = std::max(best, T.get(T.M, i, j));
		R.score = best;
		if (best == 0)
			return R;
		bool found = false;
		for (int32_t i = 1; i <= T.m && !found; i++)
			for (int32_t j = 1; j <= T.n && !found; j++)
				if (T.get(T.M, i, j) == best) {
					r = i;
					c = j;
					found = true;
				}
	} else {
		R.score = T.get(T.M, T.m, T.n);
	}
	R.lo_end = r;
	R.hi_end = c;
	if (method == SA_METHOD_NW) {
		while (r > 0 || c > 0) {
			if (r > 0 && c > 0 && T.get(T.M, r, c) == T.get(T.M, r - 1, c - 1) + sim(method, lo, hi, r, c)) {
				ops.push_back('M');
				r--, c--;
			} else if (r > 0 && T.get(T.M, r, c) == T.get(T.M, r - 1, c) + g) {
				ops.push_back('I');
				r--;
			} else {
				ops.push_back('D');
				c--;
			}
		}
	} else {
		char state = 'M';
		for (;;) {
			if (state == 'M') {
				if (method == SA_METHOD_SW && T.get(T.M, r, c) == 0)
					break;
				if (r == 0 && c == 0)
					break;
				if (r > 0 && c > 0 && T.get(T.M, r, c) == T.get(T.M, r - 1, c - 1) + sim(method, lo, hi, r, c)) {
					ops.push_back('M');
					r--, c--;
					continue;
				}
				state = T.get(T.M, r, c) == T.get(T.X, r, c) ? 'X' : 'Y';
			}
			if (state == 'X') {
				ops.push_back('D');
				state = T.get(T.X, r, c) == T.get(T.M, r, c - 1) + o ? 'M' : 'X';
				c--;
			} else {
				ops.push_back('I');
				state = T.get(T.Y, r, c) == T.get(T.M, r - 1, c) + o ? 'M' : 'Y';
				r--;
			}
			if (r < 0 || c < 0) {
				printf("literal walk left the table\n");
				exit(1);
			}
		}
	}
	R.lo_begin = r;
	R.hi_begin = c;
	R.columns = (int32_t)ops.size();
	std::reverse(ops.begin(), ops.end());
	for (size_t k = 0; k < ops.size();) {
		size_t e = k;
		while (e < ops.size() && ops[e] == ops[k])
			e++;
		int op = ops[k] == 'M' ? SA_ALN_M : ops[k] == 'I' ? SA_ALN_I : SA_ALN_D;
		if (flip && op != SA_ALN_M)
			op = op == SA_ALN_I ? SA_ALN_D : SA_ALN_I;
		R.runs.push_back((uint32_t)((e - k) << 4) | (uint32_t)op);
		k = e;
	}
	return R;
}

/* through the core: encoder -> scratch -> step + emitter */
static Result through_core(int method, const Tables &T, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t g, int32_t o,
			   bool flip, long *multi)
{
	const int64_t bytes = sa_tb_pair_bytes(T.m, T.n);
	std::vector<uint8_t> scratch((size_t)bytes, 0xff);
	/* cells in an order unlike the walk's and unlike row-major: columns descending, rows ascending */
	int32_t best = 0, br = 0, bc = 0;
	for (int32_t c = T.n; c >= 1; c--)
		for (int32_t r = 1; r <= T.m; r++) {
			const int32_t sd = T.get(T.M, r - 1, c - 1) + sim(method, lo, hi, r, c);
			uint32_t rec;
			if (method == SA_METHOD_NW)
				rec = sa_tb_encode_nw(T.get(T.M, r, c), sd, T.get(T.M, r - 1, c) + g);
			else
				rec = sa_tb_encode_affine(method == SA_METHOD_SW, T.get(T.M, r, c), sd, T.get(T.X, r, c), T.get(T.Y, r, c),
							  T.get(T.M, r, c - 1) + o, T.get(T.M, r - 1, c) + o);
			const int64_t at = sa_tb_cell_offset(T.m, r, c);
			if (at < 0 || at >= bytes || scratch[(size_t)at] != 0xff) {
				printf("cell (%d, %d) of %d x %d: offset %lld outside %lld bytes or used twice\n", r, c, T.m, T.n, (long long)at, (long long)bytes);
				exit(1);
			}
			scratch[(size_t)at] = (uint8_t)rec;
			if (method == SA_METHOD_SW && sa_tb_end_before(T.get(T.M, r, c), r, c, best, br, bc)) {
				best = T.get(T.M, r, c);
				br = r;
				bc = c;
			}
			const int32_t v = T.get(T.M, r, c);
			int ways = (v == sd) + (method == SA_METHOD_NW ? (v == T.get(T.M, r - 1, c) + g) + (v == T.get(T.M, r, c - 1) + g)
								       : (v == T.get(T.X, r, c)) + (v == T.get(T.Y, r, c)));
			*multi += ways > 1;
		}
	Result R;
	struct sa_tb_walk w = { T.m, T.n, SA_TB_STATE_M };
	R.score = T.get(T.M, T.m, T.n);
	if (method == SA_METHOD_SW) {
		w.r = br;
		w.c = bc;
		R.score = best;
	}
	const int32_t r1 = w.r, c1 = w.c;
	std::vector<uint32_t> area((size_t)(T.m + T.n));
	struct sa_tb_rle rle;
	sa_tb_rle_init(&rle, area.data() + area.size());
	for (;;) {
		const uint32_t rec = sa_tb_on_border(&w) ? 0u : scratch[(size_t)sa_tb_cell_offset(T.m, w.r, w.c)];
		const int op = sa_tb_step(&w, method, rec);
		if (op < 0)
			break;
		sa_tb_rle_push(&rle, sa_tb_mirror_op(op, flip), true);
	}
	sa_tb_rle_flush(&rle, true);
	R.columns = rle.columns;
	if (!(method == SA_METHOD_SW && rle.columns == 0)) {
		R.lo_begin = w.r;
		R.lo_end = r1;
		R.hi_begin = w.c;
		R.hi_end = c1;
	}
	R.runs.assign(area.end() - rle.runs, area.end());
	return R;
}

/* the documented scoring of a CIGAR, over the caller's (a, b) */
static int64_t rescore(int method, const Result &R, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t g, int32_t o,
		       int32_t e, bool flip)
{
	int64_t total = 0;
	int32_t r = R.lo_begin, c = R.hi_begin;
	for (uint32_t run : R.runs) {
		const int32_t len = (int32_t)(run >> 4);
		int op = (int)(run & 15);
		if (flip && op != SA_ALN_M)
			op = op == SA_ALN_I ? SA_ALN_D : SA_ALN_I; /* back to the canonical orientation */
		if (op == SA_ALN_M) {
			for (int32_t k = 0; k < len; k++, r++, c++)
				total += sim(method, lo, hi, r + 1, c + 1);
		} else {
			total += method == SA_METHOD_NW ? (int64_t)len * g : o + (int64_t)(len - 1) * std::max(o, e);
			(op == SA_ALN_I ? r : c) += len;
		}
	}
	if (r != R.lo_end || c != R.hi_end)
		return INT64_MIN;
	return total;
}

int main(int argc, char **argv)
{
	if (argc != 8) {
		fprintf(stderr, "usage: traceback_test METHOD SEED PAIRS MAXLEN ALPHABET GAP1 GAP2\n");
		return 2;
	}
	const int method = atoi(argv[1]);
	std::mt19937 rng((unsigned)atoi(argv[2]));
	const int pairs = atoi(argv[3]), maxlen = atoi(argv[4]), alphabet = atoi(argv[5]);
	const int32_t g = -atoi(argv[6]), o = -atoi(argv[6]), e = -atoi(argv[7]);
	/* a small-valued matrix that is NOT symmetric: many ties, and the index order of the two methods' lookups matters */
	for (int a = 0; a < SA_SUB_DIM; a++)
		for (int b = 0; b < SA_SUB_DIM; b++)
			S[a][b] = a == b ? 3 + a % 3 : -2 + (a * 7 + b * 3) % 4;
	long multi = 0, cells = 0, empty = 0, runs = 0;
	for (int p = 0; p < pairs; p++) {
		std::vector<uint8_t> lo((size_t)(1 + rng() % (unsigned)maxlen)), hi((size_t)(1 + rng() % (unsigned)maxlen));
		if (p == 0)
			lo.resize(1), hi.resize(1); /* length 1 x 1 */
		if (p == 1)
			lo.resize(1);
		if (p == 2)
			hi.resize(1);
		if (p == 3)
			hi.resize((size_t)std::max(maxlen, 130)); /* three strips */
		for (auto &x : lo)
			x = (uint8_t)(rng() % (unsigned)alphabet);
		for (auto &x : hi)
			x = (uint8_t)(rng() % (unsigned)alphabet);
		if (p == 4 && method == SA_METHOD_SW && alphabet >= 4) { /* S[3][1] = -2, nothing scores: best 0 */
			std::fill(lo.begin(), lo.end(), (uint8_t)1);
			std::fill(hi.begin(), hi.end(), (uint8_t)3);
		}
		const Tables T = fill(method, lo, hi, g, o, e);
		cells += (long)T.m * T.n;
		for (int flip = 0; flip < 2; flip++) {
			const Result want = literal(method, T, lo, hi, g, o, flip != 0);
			const Result got = through_core(method, T, lo, hi, g, o, flip != 0, &multi);
			if (!(got == want)) {
				printf("pair %d (%d x %d, flip %d): core and literal contract differ: score %d / %d, columns %d / %d, runs %zu / %zu\n", p, T.m,
				       T.n, flip, got.score, want.score, got.columns, want.columns, got.runs.size(), want.runs.size());
				return 1;
			}
			const int64_t again = rescore(method, got, lo, hi, g, o, e, flip != 0);
			if (again != got.score) {
				printf("pair %d (%d x %d, flip %d): the CIGAR scores %lld, the tables say %d\n", p, T.m, T.n, flip, (long long)again, got.score);
				return 1;
			}
			for (size_t k = 1; k < got.runs.size(); k++)
				if ((got.runs[k] & 15) == (got.runs[k - 1] & 15)) {
					printf("pair %d: adjacent runs share an op\n", p);
					return 1;
				}
			empty += got.columns == 0;
			runs += (long)got.runs.size();
		}
	}
	printf("traceback ok: %d pairs x 2 orders, %ld cells, %ld cells with a tie, %ld empty, %ld runs\n", pairs, cells, multi / 2, empty, runs);
	return 0;
}
