/* fit_test.cpp -- the fit contract (include/seqalign_hip.h, "queries fitted inside database sequences") on the host, built with
 * -fsanitize=address,undefined by tests/test_fit_core.py.
 *
 *   fit_test TABLE METHOD GAP_PEN GAP_OPN GAP_EXT SEED
 *       TABLE: a text file of 576 integers, the 24 x 24 substitution table, or "asym" for a built-in small-valued table that is
 *       not symmetric.  METHOD 0 NW, 1 Gotoh; the gaps in their STORED form (negated).  Pairs over alphabets of 2 .. 5 residue
 *       codes: database lengths m in {1, 2, 5, 20, 70, 130} against query lengths n in {1, 3, 8, 30, 64, 65, 130}, every
 *       combination, and further draws with m > n; in half the pairs the query is a substring of the database sequence with
 *       about one residue in ten changed.  Per pair:
 *         - the full tables are filled literally (the method's recurrences, M[r][0] = 0), the end cell is looked up by the
 *           contract's rule, and the walk takes every step through sa_tb_step_fit with the record of the cell it stands on;
 *           sa_fit_pair -- the forward recurrence the kernel runs -- must give the same score, db_begin, db_end, identities, columns;
 *         - for m <= 9 the score must equal the largest global score (a plain global recurrence of the method, its own borders)
 *           of the query against any substring of the database sequence, the empty one included.
 *       Prints counts that keep the inputs honest.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/seqalign_hip.h"
#include "../../sequencealigner_amd/csrc/sa_fit_core.h"

static const int32_t SMIN = SA_SCORE_MIN;
static int32_t S[SA_SUB_DIM * SA_SUB_DIM];

typedef std::vector<uint8_t> Seq;

struct Tables {
	int32_t m, n;
	std::vector<int32_t> M, X, Y;
	int32_t &at(std::vector<int32_t> &t, int32_t r, int32_t c) { return t[(size_t)r * (n + 1) + c]; }
	int32_t get(const std::vector<int32_t> &t, int32_t r, int32_t c) const { return t[(size_t)r * (n + 1) + c]; }
};

/* S of cell (r, c) as the score kernels index it: NW sub[row][column], Gotoh sub[column][row] */
static int32_t sim(int method, const Seq &db, const Seq &qy, int32_t r, int32_t c)
{
	return method == SA_METHOD_NW ? S[db[r - 1] * SA_SUB_DIM + qy[c - 1]] : S[qy[c - 1] * SA_SUB_DIM + db[r - 1]];
}

/* fit = true: column 0 of M is 0; false: the method's own global tables, borders filled as nw.c:14-20 / ga.c:23-38 fill them */
static Tables fill(int method, bool fit, const Seq &db, const Seq &qy, int32_t g, int32_t o, int32_t e)
{
	Tables T;
	T.m = (int32_t)db.size();
	T.n = (int32_t)qy.size();
	const size_t cells = (size_t)(T.m + 1) * (T.n + 1);
	T.M.assign(cells, 0);
	T.X.assign(cells, SMIN);
	T.Y.assign(cells, SMIN);
	if (method == SA_METHOD_NW) {
		for (int32_t c = 0; c <= T.n; c++)
			T.at(T.M, 0, c) = c * g;
		for (int32_t r = 1; r <= T.m; r++)
			T.at(T.M, r, 0) = fit ? 0 : r * g;
	} else {
		int32_t x = SMIN;
		for (int32_t c = 1; c <= T.n; c++) { /* (the row-0 values of X are M's; no interior cell reads them as X) */
			x = std::max(T.get(T.M, 0, c - 1) + o, x + e);
			T.at(T.M, 0, c) = x;
		}
		int32_t y = SMIN;
		for (int32_t r = 1; r <= T.m; r++) {
			y = std::max(T.get(T.M, r - 1, 0) + o, y + e);
			T.at(T.M, r, 0) = fit ? 0 : y;
			if (fit)
				y = SMIN; /* (never read: M[r - 1][0] + o is taken from the table) */
		}
	}
	for (int32_t r = 1; r <= T.m; r++)
		for (int32_t c = 1; c <= T.n; c++) {
			const int32_t sd = T.get(T.M, r - 1, c - 1) + sim(method, db, qy, r, c);
			if (method == SA_METHOD_NW) {
				T.at(T.M, r, c) = std::max(T.get(T.M, r, c - 1) + g, std::max(T.get(T.M, r - 1, c) + g, sd));
				continue;
			}
			const int32_t x = std::max(T.get(T.M, r, c - 1) + o, T.get(T.X, r, c - 1) + e);
			const int32_t y = std::max(T.get(T.M, r - 1, c) + o, T.get(T.Y, r - 1, c) + e);
			T.at(T.X, r, c) = x;
			T.at(T.Y, r, c) = y;
			T.at(T.M, r, c) = std::max(y, std::max(x, sd));
		}
	return T;
}

struct Result {
	int32_t score = 0, db_begin = 0, db_end = 0, identities = 0, columns = 0, gaps = 0; /* gaps: I and D columns */
};

/* the record of an interior cell, from the full tables */
static uint32_t record(int method, const Tables &T, const Seq &db, const Seq &qy, int32_t g, int32_t o, int32_t r, int32_t c)
{
	const int32_t sd = T.get(T.M, r - 1, c - 1) + sim(method, db, qy, r, c);
	if (method == SA_METHOD_NW)
		return sa_tb_encode_nw(T.get(T.M, r, c), sd, T.get(T.M, r - 1, c) + g);
	return sa_tb_encode_affine(false, T.get(T.M, r, c), sd, T.get(T.X, r, c), T.get(T.Y, r, c), T.get(T.M, r, c - 1) + o, T.get(T.M, r - 1, c) + o);
}

/* end cell and walk of the fit contract over the full tables */
static Result walk(int method, const Tables &T, const Seq &db, const Seq &qy, int32_t g, int32_t o)
{
	Result R;
	int32_t end = 0;
	for (int32_t r = 1; r <= T.m; r++) /* the largest M of column n, the smallest r on a tie */
		if (T.get(T.M, r, T.n) > T.get(T.M, end, T.n))
			end = r;
	R.score = T.get(T.M, end, T.n);
	R.db_end = end;
	struct sa_tb_walk w = { end, T.n, SA_TB_STATE_M };
	for (;;) {
		const int32_t r = w.r, c = w.c;
		const uint32_t rec = (r == 0 || c == 0) ? 0u : record(method, T, db, qy, g, o, r, c);
		const int op = sa_tb_step_fit(&w, method, rec);
		if (op < 0)
			break;
		R.columns++;
		if (op == SA_TB_OP_M)
			R.identities += db[r - 1] == qy[c - 1];
		else
			R.gaps++;
		if (w.r < 0 || w.c < 0) {
			printf("the walk left the table\n");
			exit(1);
		}
	}
	if (w.c != 0) {
		printf("the walk stopped at column %d\n", w.c);
		exit(1);
	}
	R.db_begin = w.r;
	return R;
}

/* the largest global score of the query against any substring of db; the empty substring in closed form */
static int32_t brute(int method, const Seq &db, const Seq &qy, int32_t g, int32_t o, int32_t e)
{
	int32_t best = sa_fit_border(method, (int32_t)qy.size(), g, o, e);
	for (size_t s = 0; s < db.size(); s++)
		for (size_t t = s + 1; t <= db.size(); t++) {
			const Seq part(db.begin() + (long)s, db.begin() + (long)t);
			const Tables T = fill(method, false, part, qy, g, o, e);
			best = std::max(best, T.get(T.M, T.m, T.n));
		}
	return best;
}

int main(int argc, char **argv)
{
	if (argc != 7) {
		fprintf(stderr, "usage: fit_test TABLE METHOD GAP_PEN GAP_OPN GAP_EXT SEED\n");
		return 2;
	}
	if (!strcmp(argv[1], "asym")) {
		for (int a = 0; a < SA_SUB_DIM; a++)
			for (int b = 0; b < SA_SUB_DIM; b++)
				S[a * SA_SUB_DIM + b] = a == b ? 3 + a % 3 : -2 + (a * 7 + b * 3) % 4;
	} else {
		FILE *f = fopen(argv[1], "r");
		if (!f) {
			fprintf(stderr, "cannot open %s\n", argv[1]);
			return 2;
		}
		for (int k = 0; k < SA_SUB_DIM * SA_SUB_DIM; k++)
			if (fscanf(f, "%d", &S[k]) != 1) {
				fprintf(stderr, "%s: entry %d missing\n", argv[1], k);
				fclose(f);
				return 2;
			}
		fclose(f);
	}
	const int method = atoi(argv[2]);
	if (method != SA_METHOD_NW && method != SA_METHOD_GA) {
		fprintf(stderr, "METHOD must be 0 (NW) or 1 (Gotoh)\n");
		return 2;
	}
	const int32_t g = atoi(argv[3]), o = atoi(argv[4]), e = atoi(argv[5]);
	std::mt19937 rng((unsigned)atoi(argv[6]));
	static const int DB_LENS[] = { 1, 2, 5, 20, 70, 130 };
	static const int QY_LENS[] = { 1, 3, 8, 30, 64, 65, 130 };
	long pairs = 0, end0 = 0, shorter = 0, inside = 0, gapped = 0, brute_checked = 0, planted = 0;
	auto one = [&](size_t m, size_t n, unsigned alphabet, bool plant) {
		Seq db(m), qy(n);
		/* residue codes C, E, W, I, A: under BLOSUM62 the pair C / E scores -4, no better than a gap of the scorings tested */
		static const uint8_t CODES[] = { 4, 6, 17, 9, 0 };
		for (auto &x : db)
			x = CODES[rng() % alphabet];
		for (auto &x : qy)
			x = CODES[rng() % alphabet];
		if (plant && n <= m) { /* the query is db[s, s + n) with about one residue in ten changed; strictly inside where there is room */
			const size_t room = m - n, s = room >= 2 ? 1 + rng() % (room - 1) : rng() % (room + 1);
			for (size_t k = 0; k < n; k++)
				qy[k] = rng() % 10 ? db[s + k] : qy[k];
			planted++;
		}
		const Tables T = fill(method, true, db, qy, g, o, e);
		const Result want = walk(method, T, db, qy, g, o);
		std::vector<int32_t> vals(3 * (n + 1));
		std::vector<sa_fit_pay> pays(3 * (n + 1));
		const sa_fit_result got = sa_fit_pair(method, db.data(), (int32_t)m, qy.data(), (int32_t)n, S, g, o, e, vals.data(), pays.data());
		if (got.score != want.score || got.db_begin != want.db_begin || got.db_end != want.db_end || got.identities != want.identities ||
		    got.columns != want.columns) {
			printf("pair %ld (%zu x %zu, alphabet %u): forward (score %d, span [%d, %d), identities %d, columns %d), walk (%d, [%d, %d), %d, %d)\n",
			       pairs, m, n, alphabet, got.score, got.db_begin, got.db_end, got.identities, got.columns, want.score, want.db_begin, want.db_end,
			       want.identities, want.columns);
			exit(1);
		}
		if (want.db_begin < 0 || want.db_begin > want.db_end || want.db_end > (int32_t)m) {
			printf("pair %ld: span [%d, %d) of %zu\n", pairs, want.db_begin, want.db_end, m);
			exit(1);
		}
		if (m <= 9) {
			const int32_t b = brute(method, db, qy, g, o, e);
			if (b != want.score) {
				printf("pair %ld (%zu x %zu, alphabet %u): fit score %d, the best substring scores %d\n", pairs, m, n, alphabet, want.score, b);
				exit(1);
			}
			brute_checked++;
		}
		pairs++;
		end0 += want.db_end == 0;
		shorter += m < n;
		inside += want.db_begin > 0 && want.db_end < (int32_t)m;
		gapped += want.gaps > 0;
	};
	for (unsigned alphabet = 2; alphabet <= 5; alphabet++) {
		for (int rep = 0; rep < 2; rep++)
			for (int m : DB_LENS)
				for (int n : QY_LENS)
					one((size_t)m, (size_t)n, alphabet, (pairs & 1) != 0);
		for (int k = 0; k < 80; k++) { /* further draws from the same lengths with room around the query */
			const int m = DB_LENS[3 + rng() % 3];
			int n;
			do
				n = QY_LENS[rng() % 7];
			while (n + 2 > m);
			one((size_t)m, (size_t)n, alphabet, (pairs & 1) != 0);
		}
	}
	printf("fit ok: %ld pairs, %ld end row 0, %ld m < n, %ld inside, %ld with gaps, %ld against brute force, %ld planted\n", pairs, end0, shorter,
	       inside, gapped, brute_checked, planted);
	return 0;
}
