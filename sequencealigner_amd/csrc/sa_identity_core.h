/* sa_identity_core.h -- what the identity kernel (sa_identity.hip) and the host share: the payload a DP state carries forward,
 * its three update rules, the percent-identity arithmetic and a serial full-table restatement.  Plain C++ that the host compiles
 * as well: tests/host_c/identity_test.cpp runs it under ASan / UBSan against a literal fill + walk of the traceback contract.
 *
 * Contract (include/seqalign_hip.h, "percent identity of every pair"), in the canonical orientation of the alignment contract:
 * the canonical optimal alignment of a pair is a per-cell function of the DP tables, so (identities, columns) of the canonical
 * path that ENDS in a state of a cell follow from the payloads of the states that path comes from:
 *   borders  NW / Gotoh: P(0, c) = (0, c), P(r, 0) = (0, r) in every state (the walk goes left along row 0 and up along
 *            column 0, one column per step, no M column); SW: (0, 0) (the walk stops on a border)
 *   NW       record of sa_tb_encode_nw:  DIAG: P[r-1][c-1] + (equal, 1);  Y (up): P[r-1][c] + (0, 1);  X (left): P[r][c-1] + (0, 1)
 *   affine   record of sa_tb_encode_affine:
 *            PX[r][c] = (XOPEN ? PM[r][c-1] : PX[r][c-1]) + (0, 1)
 *            PY[r][c] = (YOPEN ? PM[r-1][c] : PY[r-1][c]) + (0, 1)
 *            PM[r][c]: STOP: (0, 0);  DIAG: PM[r-1][c-1] + (equal, 1);  X: PX[r][c];  Y: PY[r][c]
 *   result   NW / Gotoh: PM[m][n];  SW: PM at the end cell of sa_tb_end_before (best == 0: (0, 0))
 * Every decision is taken from the record of sa_traceback_core.h: the tie rule exists in one place. */
#ifndef SA_IDENTITY_CORE_H
#define SA_IDENTITY_CORE_H

#include <stdint.h>

#include "sa_traceback_core.h"

enum { SA_ID_DENOM_COLUMNS = 0, SA_ID_DENOM_SHORTER = 1, SA_ID_DENOM_LONGER = 2, SA_ID_DENOM_MEAN = 3 }; /* = SA_PID_* */
#define SA_ID_PPM 1000000 /* = SA_NORM_SCALE */
#define SA_ID_SCORE_MIN (INT32_MIN / 2) /* reference src/bio/align.h:19 */

/* the payload of one state of one cell: M columns with equal residue codes, and columns, of the canonical path that ends there */
struct sa_id_pay {
	int32_t identities, columns;
};

static inline SA_TB_HD struct sa_id_pay sa_id_make(int32_t identities, int32_t columns)
{
	struct sa_id_pay p = { identities, columns };
	return p;
}

/* one more column; `equal`: it is an M column whose two residue codes are equal */
static inline SA_TB_HD struct sa_id_pay sa_id_add(struct sa_id_pay p, bool equal)
{
	return sa_id_make(p.identities + (equal ? 1 : 0), p.columns + 1);
}

/* border payload of cell (0, k) or (k, 0) */
static inline SA_TB_HD struct sa_id_pay sa_id_border(int method, int32_t k) { return sa_id_make(0, method == SA_TB_SW ? 0 : k); }

/* NW: rec = sa_tb_encode_nw(...); diag = P[r-1][c-1], up = P[r-1][c], left = P[r][c-1] */
static inline SA_TB_HD struct sa_id_pay sa_id_step_nw(uint32_t rec, bool equal, struct sa_id_pay diag, struct sa_id_pay up, struct sa_id_pay left)
{
	const uint32_t choice = rec & 3u;
	return choice == SA_TB_DIAG ? sa_id_add(diag, equal) : choice == SA_TB_Y ? sa_id_add(up, false) : sa_id_add(left, false);
}

/* Gotoh / SW: rec = sa_tb_encode_affine(...) */
static inline SA_TB_HD struct sa_id_pay sa_id_step_x(uint32_t rec, struct sa_id_pay left_m, struct sa_id_pay left_x)
{
	return sa_id_add((rec & SA_TB_XOPEN) ? left_m : left_x, false);
}

static inline SA_TB_HD struct sa_id_pay sa_id_step_y(uint32_t rec, struct sa_id_pay up_m, struct sa_id_pay up_y)
{
	return sa_id_add((rec & SA_TB_YOPEN) ? up_m : up_y, false);
}

/* px, py: the payloads of X and Y of THIS cell (sa_id_step_x / _y) */
static inline SA_TB_HD struct sa_id_pay sa_id_step_m(uint32_t rec, bool equal, struct sa_id_pay diag_m, struct sa_id_pay px, struct sa_id_pay py)
{
	const uint32_t choice = rec & 3u;
	return choice == SA_TB_STOP ? sa_id_make(0, 0) : choice == SA_TB_DIAG ? sa_id_add(diag_m, equal) : choice == SA_TB_X ? px : py;
}

/* ---- percent identity in parts per million: exact, 64-bit (0 <= identities <= D <= 2^32 in every use) ---------------------- */
static inline SA_TB_HD bool sa_id_denom_ok(int32_t denom) { return denom >= SA_ID_DENOM_COLUMNS && denom <= SA_ID_DENOM_MEAN; }

/* D <= 0: INT32_MIN.  Otherwise floor(num / D) (num >= 0 for identities >= 0; a negative num, which no alignment gives, floors
 * towards minus infinity as sa_norm_value does), saturated to int32. */
static inline SA_TB_HD int32_t sa_id_pid(int32_t identities, int32_t columns, int32_t len_i, int32_t len_j, int32_t denom)
{
	int64_t D, num = (int64_t)identities * SA_ID_PPM;
	if (denom == SA_ID_DENOM_COLUMNS)
		D = columns;
	else if (denom == SA_ID_DENOM_SHORTER)
		D = len_i < len_j ? len_i : len_j;
	else if (denom == SA_ID_DENOM_LONGER)
		D = len_i > len_j ? len_i : len_j;
	else {
		D = (int64_t)len_i + len_j;
		num *= 2;
	}
	if (D <= 0)
		return INT32_MIN;
	int64_t q = num / D;
	if (num % D != 0 && num < 0)
		q--;
	return q < INT32_MIN ? INT32_MIN : q > INT32_MAX ? INT32_MAX : (int32_t)q;
}

/* ---- serial restatement over full rows: what one wavefront of sa_k_identity computes for a pair ---------------------------
 * lo[0 .. m) the codes of the row sequence, hi[0 .. n) of the column sequence, sub the 24 x 24 table indexed as the score
 * kernels index it (NW [lo][hi], Gotoh / SW [hi][lo]); one row of each table is kept, in scratch the caller owns:
 * vals int32[3 * (n + 1)], pays sa_id_pay[3 * (n + 1)].  Returns the score; *out = (identities, columns). */
static inline SA_TB_HD int32_t sa_id_pair(int method, const uint8_t *lo, int32_t m, const uint8_t *hi, int32_t n, const int32_t *sub, int32_t g,
					  int32_t o, int32_t e, int32_t *vals, struct sa_id_pay *pays, struct sa_id_pay *out)
{
	int32_t *M = vals, *X = vals + (n + 1), *Y = vals + 2 * (n + 1);
	struct sa_id_pay *PM = pays, *PX = pays + (n + 1), *PY = pays + 2 * (n + 1);
	const int32_t ga_b1 = o > SA_ID_SCORE_MIN + e ? o : SA_ID_SCORE_MIN + e, ga_w = o > e ? o : e;
	/* row 0 */
	for (int32_t c = 0; c <= n; c++) {
		M[c] = method == SA_TB_NW ? c * g : method == SA_TB_GA ? (c == 0 ? 0 : ga_b1 + (c - 1) * ga_w) : 0;
		X[c] = Y[c] = SA_ID_SCORE_MIN;
		PM[c] = PX[c] = PY[c] = sa_id_border(method, c);
	}
	int32_t best = 0, best_r = 0, best_c = 0;
	struct sa_id_pay best_p = sa_id_make(0, 0);
	for (int32_t r = 1; r <= m; r++) {
		const int32_t a = lo[r - 1];
		/* column 0 of this row; the values of row r - 1, column c - 1 travel in d* */
		int32_t dM = M[0];
		struct sa_id_pay dPM = PM[0];
		M[0] = method == SA_TB_NW ? r * g : method == SA_TB_GA ? ga_b1 + (r - 1) * ga_w : 0;
		X[0] = SA_ID_SCORE_MIN;
		PM[0] = PX[0] = PY[0] = sa_id_border(method, r);
		for (int32_t c = 1; c <= n; c++) {
			const int32_t b = hi[c - 1];
			const bool equal = a == b;
			const int32_t upM = M[c], upY = Y[c];
			const struct sa_id_pay upPM = PM[c], upPY = PY[c];
			int32_t nm;
			struct sa_id_pay pm;
			if (method == SA_TB_NW) {
				const int32_t match = dM + sub[a * 24 + b], del = upM + g, ins = M[c - 1] + g;
				nm = ins > del ? ins : del;
				nm = nm > match ? nm : match;
				pm = sa_id_step_nw(sa_tb_encode_nw(nm, match, del), equal, dPM, upPM, PM[c - 1]);
			} else {
				const int32_t sd = dM + sub[b * 24 + a];
				const int32_t xo = M[c - 1] + o, yo = upM + o;
				const int32_t xe = X[c - 1] + e, ye = upY + e;
				const int32_t nx = xo > xe ? xo : xe, ny = yo > ye ? yo : ye;
				nm = method == SA_TB_SW && sd < 0 ? 0 : sd;
				nm = nx > nm ? nx : nm;
				nm = ny > nm ? ny : nm;
				const uint32_t rec = sa_tb_encode_affine(method == SA_TB_SW, nm, sd, nx, ny, xo, yo);
				const struct sa_id_pay px = sa_id_step_x(rec, PM[c - 1], PX[c - 1]);
				const struct sa_id_pay py = sa_id_step_y(rec, upPM, upPY);
				pm = sa_id_step_m(rec, equal, dPM, px, py);
				X[c] = nx;
				Y[c] = ny;
				PX[c] = px;
				PY[c] = py;
			}
			dM = upM;
			dPM = upPM;
			M[c] = nm;
			PM[c] = pm;
			if (method == SA_TB_SW && sa_tb_end_before(nm, r, c, best, best_r, best_c)) {
				best = nm;
				best_r = r;
				best_c = c;
				best_p = pm;
			}
		}
	}
	if (method == SA_TB_SW) {
		*out = best_p;
		return best;
	}
	*out = PM[n];
	return M[n];
}

#endif /* SA_IDENTITY_CORE_H */
