/* identity_test.cpp -- the identity contract (include/seqalign_hip.h, "percent identity of every pair") on the host, built with
 * -fsanitize=address,undefined by tests/test_identity_core.py.
 *
 *   identity_test --pairs TABLE METHOD GAP_PEN GAP_OPN GAP_EXT SEED
 *       TABLE: a text file of 576 integers, the 24 x 24 substitution table, or "asym" for a built-in small-valued table that is
 *       not symmetric.  METHOD 0 NW, 1 Gotoh, 2 SW; the gaps in their STORED form (negated).  Random pairs over alphabets of
 *       2 .. 5 residue codes: lengths 1 .. 14, and the strip edges 63 / 64 / 65 / 129 against each other and against short
 *       ones.  Per pair: the full tables are filled with the reference's recurrences (nw.c, ga.c, sw.c); the walk of the
 *       alignment contract starts at the end cell and takes every step through sa_tb_step with the record of the cell it stands
 *       on, counting columns and the M columns with equal codes; sa_id_pair -- the forward recurrence the kernel runs -- must
 *       give the same score, identities and columns.
 *   identity_test --pid
 *       sa_id_pid against 128-bit arithmetic: identities 0, D - 1 and D, D = 0, lengths 1 and INT32_MAX / 2, every denominator.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/seqalign_hip.h"
#include "../../sequencealigner_amd/csrc/sa_identity_core.h"

static const int32_t SMIN = SA_SCORE_MIN;
static int32_t S[SA_SUB_DIM * SA_SUB_DIM];

struct Tables {
	int32_t m, n;
	std::vector<int32_t> M, X, Y;
	int32_t &at(std::vector<int32_t> &t, int32_t r, int32_t c) { return t[(size_t)r * (n + 1) + c]; }
	int32_t get(const std::vector<int32_t> &t, int32_t r, int32_t c) const { return t[(size_t)r * (n + 1) + c]; }
};

/* S of cell (r, c) as the score kernels index it: NW sub[lo][hi], Gotoh / SW sub[hi][lo] */
static int32_t sim(int method, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t r, int32_t c)
{
	return method == SA_METHOD_NW ? S[lo[r - 1] * SA_SUB_DIM + hi[c - 1]] : S[hi[c - 1] * SA_SUB_DIM + lo[r - 1]];
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
	int32_t score = 0, identities = 0, columns = 0, gaps = 0; /* gaps: I and D columns */
};

/* the record of an interior cell, from the full tables */
static uint32_t record(int method, const Tables &T, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t g, int32_t o, int32_t r,
		       int32_t c)
{
	const int32_t sd = T.get(T.M, r - 1, c - 1) + sim(method, lo, hi, r, c);
	if (method == SA_METHOD_NW)
		return sa_tb_encode_nw(T.get(T.M, r, c), sd, T.get(T.M, r - 1, c) + g);
	return sa_tb_encode_affine(method == SA_METHOD_SW, T.get(T.M, r, c), sd, T.get(T.X, r, c), T.get(T.Y, r, c), T.get(T.M, r, c - 1) + o,
				   T.get(T.M, r - 1, c) + o);
}

/* the walk of the alignment contract over the full tables */
static Result walk(int method, const Tables &T, const std::vector<uint8_t> &lo, const std::vector<uint8_t> &hi, int32_t g, int32_t o)
{
	Result R;
	struct sa_tb_walk w = { T.m, T.n, SA_TB_STATE_M };
	R.score = T.get(T.M, T.m, T.n);
	if (method == SA_METHOD_SW) {
		int32_t best = 0;
		for (int32_t r = 1; r <= T.m; r++)
			for (int32_t c = 1; c <= T.n; c++)
				best = std::max(best, T.get(T.M, r, c));
		R.score = best;
		if (best == 0)
			return R;
		bool found = false;
		for (int32_t r = 1; r <= T.m && !found; r++) /* smallest r, then smallest c */
			for (int32_t c = 1; c <= T.n && !found; c++)
				if (T.get(T.M, r, c) == best) {
					w.r = r;
					w.c = c;
					found = true;
				}
	}
	for (;;) {
		const int32_t r = w.r, c = w.c;
		const uint32_t rec = sa_tb_on_border(&w) ? 0u : record(method, T, lo, hi, g, o, r, c);
		const int op = sa_tb_step(&w, method, rec);
		if (op < 0)
			break;
		R.columns++;
		if (op == SA_TB_OP_M)
			R.identities += lo[r - 1] == hi[c - 1];
		else
			R.gaps++;
		if (w.r < 0 || w.c < 0) {
			printf("the walk left the table\n");
			exit(1);
		}
	}
	return R;
}

static int run_pairs(int argc, char **argv)
{
	if (argc != 8) {
		fprintf(stderr, "usage: identity_test --pairs TABLE METHOD GAP_PEN GAP_OPN GAP_EXT SEED\n");
		return 2;
	}
	if (!strcmp(argv[2], "asym")) {
		for (int a = 0; a < SA_SUB_DIM; a++)
			for (int b = 0; b < SA_SUB_DIM; b++)
				S[a * SA_SUB_DIM + b] = a == b ? 3 + a % 3 : -2 + (a * 7 + b * 3) % 4;
	} else {
		FILE *f = fopen(argv[2], "r");
		if (!f) {
			fprintf(stderr, "cannot open %s\n", argv[2]);
			return 2;
		}
		for (int k = 0; k < SA_SUB_DIM * SA_SUB_DIM; k++)
			if (fscanf(f, "%d", &S[k]) != 1) {
				fprintf(stderr, "%s: entry %d missing\n", argv[2], k);
				fclose(f);
				return 2;
			}
		fclose(f);
	}
	const int method = atoi(argv[3]);
	const int32_t g = atoi(argv[4]), o = atoi(argv[5]), e = atoi(argv[6]);
	std::mt19937 rng((unsigned)atoi(argv[7]));
	static const int EDGES[] = { 63, 64, 65, 129 };
	long pairs = 0, cells = 0, empty = 0, gapped = 0, identities = 0;
	auto one = [&](size_t m, size_t n, unsigned alphabet) {
		std::vector<uint8_t> lo(m), hi(n);
		for (auto &x : lo)
			x = (uint8_t)(rng() % alphabet);
		for (auto &x : hi)
			x = (uint8_t)(rng() % alphabet);
		if (rng() % 4 == 0 && n >= m) /* a near-copy: long diagonals with a few changes */
			for (size_t k = 0; k < m; k++)
				hi[k + (n - m) / 2] = rng() % 8 ? lo[k] : hi[k + (n - m) / 2];
		const Tables T = fill(method, lo, hi, g, o, e);
		const Result want = walk(method, T, lo, hi, g, o);
		std::vector<int32_t> vals(3 * (n + 1));
		std::vector<sa_id_pay> pays(3 * (n + 1));
		sa_id_pay got = { -1, -1 };
		const int32_t score = sa_id_pair(method, lo.data(), (int32_t)m, hi.data(), (int32_t)n, S, g, o, e, vals.data(), pays.data(), &got);
		if (score != want.score || got.identities != want.identities || got.columns != want.columns) {
			printf("pair %ld (%zu x %zu, alphabet %u): forward (score %d, identities %d, columns %d), walk (%d, %d, %d)\n", pairs, m, n, alphabet,
			       score, got.identities, got.columns, want.score, want.identities, want.columns);
			exit(1);
		}
		pairs++;
		cells += (long)(m * n);
		empty += want.columns == 0;
		gapped += want.gaps > 0;
		identities += want.identities;
	};
	for (unsigned alphabet = 2; alphabet <= 5; alphabet++) {
		for (int k = 0; k < 150; k++)
			one(1 + rng() % 14, 1 + rng() % 14, alphabet);
		for (int a : EDGES)
			for (int b : EDGES)
				one((size_t)a, (size_t)b, alphabet);
		for (int a : EDGES) {
			one((size_t)a, 1 + rng() % 14, alphabet);
			one(1 + rng() % 14, (size_t)a, alphabet);
		}
		one(1, 1, alphabet);
	}
	printf("identity ok: %ld pairs, %ld cells, %ld empty, %ld with gaps, %ld identities\n", pairs, cells, empty, gapped, identities);
	return 0;
}

static int32_t wide_pid(int64_t identities, int64_t columns, int64_t li, int64_t lj, int denom)
{
	__int128 D, num = (__int128)identities * 1000000;
	if (denom == SA_PID_COLUMNS)
		D = columns;
	else if (denom == SA_PID_SHORTER)
		D = std::min(li, lj);
	else if (denom == SA_PID_LONGER)
		D = std::max(li, lj);
	else {
		D = (__int128)li + lj;
		num *= 2;
	}
	if (D <= 0)
		return INT32_MIN;
	__int128 q = num / D;
	if (num % D != 0 && num < 0)
		q--;
	return (int32_t)std::max<__int128>(INT32_MIN, std::min<__int128>(INT32_MAX, q));
}

static int run_pid()
{
	static const int32_t LENS[] = { 1, 2, 3, 7, 100, 12345, INT32_MAX / 2 - 1, INT32_MAX / 2 };
	long checked = 0, full = 0, undefined = 0;
	for (int denom = SA_PID_COLUMNS; denom <= SA_PID_MEAN; denom++)
		for (int32_t li : LENS)
			for (int32_t lj : LENS) {
				const int32_t shorter = std::min(li, lj);
				/* columns between the longer length and the sum of both; 0: the empty SW alignment */
				const int32_t cols[] = { 0, std::max(li, lj), (int32_t)std::min<int64_t>((int64_t)li + lj, INT32_MAX) };
				for (int32_t c : cols) {
					const int32_t top = c == 0 ? 0 : std::min(shorter, c); /* identities never exceed the shorter sequence */
					const int32_t ids[] = { 0, top > 0 ? top - 1 : 0, top, top / 2, top / 3 };
					for (int32_t id : ids) {
						const int32_t got = sa_id_pid(id, c, li, lj, denom), want = wide_pid(id, c, li, lj, denom);
						if (got != want) {
							printf("pid(%d, %d, %d, %d, denom %d) = %d, 128-bit arithmetic says %d\n", id, c, li, lj, denom, got, want);
							return 1;
						}
						if (want != INT32_MIN && (want < 0 || want > 1000000)) {
							printf("pid(%d, %d, %d, %d, denom %d) = %d is outside [0, 1000000]\n", id, c, li, lj, denom, want);
							return 1;
						}
						checked++;
						full += want == 1000000;
						undefined += want == INT32_MIN;
					}
				}
			}
	if (sa_id_denom_ok(-1) || sa_id_denom_ok(4) || !sa_id_denom_ok(0) || !sa_id_denom_ok(3)) {
		printf("sa_id_denom_ok disagrees with the enum\n");
		return 1;
	}
	printf("pid ok: %ld values, %ld at 1000000, %ld undefined\n", checked, full, undefined);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "--pairs"))
		return run_pairs(argc, argv);
	if (argc == 2 && !strcmp(argv[1], "--pid"))
		return run_pid();
	fprintf(stderr, "usage: identity_test --pairs TABLE METHOD GAP_PEN GAP_OPN GAP_EXT SEED | --pid\n");
	return 2;
}
