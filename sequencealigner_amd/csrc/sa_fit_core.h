/* sa_fit_core.h -- what the fit kernel (sa_fit.hip) and the host share: the payload a DP state carries forward under the fit
 * contract, its update rules, the end-cell comparison, the walk step and a serial restatement over rolling rows.  Plain C++
 * that the host compiles as well: tests/host_c/fit_test.cpp runs it under ASan / UBSan against a literal full-table fill plus
 * the contract's walk, and against the brute-force maximum over the substrings of the database sequence.
 *
 * Contract (include/seqalign_hip.h, "queries fitted inside database sequences"), canonical orientation: the database sequence
 * (length m) is the row sequence, the query (length n) the column sequence.  The tables are the method's (NW, Gotoh) with one
 * difference, M[r][0] = 0 for every r: leaving the database's first residues costs nothing.  Among the cells (r, n) the
 * largest M wins, the smallest r on a tie (row 0 takes part); the walk starts there in state M, stops at c == 0 (db_begin = r
 * there), goes left along row 0 and takes every other step as sa_tb_step does.
 *   payload  (identities, columns, begin) of the canonical path that ENDS in a state of a cell: identities and columns by the
 *            rules of sa_identity_core.h, begin carried along unchanged
 *   borders  P(r, 0) = (0, 0, r), P(0, c) = (0, c, 0), in every state
 *   result   PM at the end cell
 * Every decision is taken from the record of sa_traceback_core.h: the tie rule exists in one place. */
#ifndef SA_FIT_CORE_H
#define SA_FIT_CORE_H

#include <stdint.h>

#include "sa_identity_core.h"

struct sa_fit_pay {
	int32_t identities, columns, begin;
};

static inline SA_TB_HD struct sa_fit_pay sa_fit_make(int32_t identities, int32_t columns, int32_t begin)
{
	struct sa_fit_pay p = { identities, columns, begin };
	return p;
}

/* one more column; `equal`: it is an M column whose two residue codes are equal */
static inline SA_TB_HD struct sa_fit_pay sa_fit_add(struct sa_fit_pay p, bool equal)
{
	return sa_fit_make(p.identities + (equal ? 1 : 0), p.columns + 1, p.begin);
}

static inline SA_TB_HD struct sa_fit_pay sa_fit_border_row0(int32_t c) { return sa_fit_make(0, c, 0); } /* P(0, c) */
static inline SA_TB_HD struct sa_fit_pay sa_fit_border_col0(int32_t r) { return sa_fit_make(0, 0, r); } /* P(r, 0) */

/* the rules of sa_id_step_nw / _x / _y / _m on the wider payload (no STOP: SW is not a fit method) */
static inline SA_TB_HD struct sa_fit_pay sa_fit_step_nw(uint32_t rec, bool equal, struct sa_fit_pay diag, struct sa_fit_pay up, struct sa_fit_pay left)
{
	const uint32_t choice = rec & 3u;
	return choice == SA_TB_DIAG ? sa_fit_add(diag, equal) : choice == SA_TB_Y ? sa_fit_add(up, false) : sa_fit_add(left, false);
}

static inline SA_TB_HD struct sa_fit_pay sa_fit_step_x(uint32_t rec, struct sa_fit_pay left_m, struct sa_fit_pay left_x)
{
	return sa_fit_add((rec & SA_TB_XOPEN) ? left_m : left_x, false);
}

static inline SA_TB_HD struct sa_fit_pay sa_fit_step_y(uint32_t rec, struct sa_fit_pay up_m, struct sa_fit_pay up_y)
{
	return sa_fit_add((rec & SA_TB_YOPEN) ? up_m : up_y, false);
}

/* px, py: the payloads of X and Y of THIS cell */
static inline SA_TB_HD struct sa_fit_pay sa_fit_step_m(uint32_t rec, bool equal, struct sa_fit_pay diag_m, struct sa_fit_pay px, struct sa_fit_pay py)
{
	const uint32_t choice = rec & 3u;
	return choice == SA_TB_DIAG ? sa_fit_add(diag_m, equal) : choice == SA_TB_X ? px : py;
}

/* end cell: does (v, r) come before (bv, br) under the key (M descending, r ascending)? */
static inline SA_TB_HD bool sa_fit_end_before(int32_t v, int32_t r, int32_t bv, int32_t br) { return v > bv || (v == bv && r < br); }

/* row-0 value of the method: M[0][k] (nw.c:16-20, ga.c:26-38 in closed form) */
static inline SA_TB_HD int32_t sa_fit_border(int method, int32_t k, int32_t g, int32_t o, int32_t e)
{
	if (method == SA_TB_NW)
		return k * g;
	const int32_t b1 = o > SA_ID_SCORE_MIN + e ? o : SA_ID_SCORE_MIN + e, w = o > e ? o : e;
	return k == 0 ? 0 : b1 + (k - 1) * w;
}

/* One step of the fit walk from the cell it stands on; `rec` is that cell's record (not read where r == 0 or c == 0).  Returns
 * the op of the column it emits (SA_TB_OP_*: I a residue of the database sequence only, D of the query only, as sa_tb_step
 * names them in the canonical orientation), or -1: the walk is over, c == 0 and r is db_begin. */
static inline SA_TB_HD int sa_tb_step_fit(struct sa_tb_walk *w, int method, uint32_t rec)
{
	if (w->c == 0)
		return -1;
	if (w->r == 0) {
		w->state = SA_TB_STATE_M;
		w->c--;
		return SA_TB_OP_D;
	}
	return sa_tb_step(w, method, rec);
}

struct sa_fit_result {
	int32_t score, db_begin, db_end, identities, columns;
};

/* ---- serial restatement over rolling rows: what one wavefront of sa_k_fit computes for a pair --------------------------------
 * db[0 .. m) the codes of the database sequence (rows), qy[0 .. n) of the query (columns), sub the 24 x 24 table indexed as the
 * score kernels index it (NW [db][qy], Gotoh [qy][db]); one row of each table is kept, in scratch the caller owns:
 * vals int32[3 * (n + 1)], pays sa_fit_pay[3 * (n + 1)].  method: SA_TB_NW or SA_TB_GA. */
static inline SA_TB_HD struct sa_fit_result sa_fit_pair(int method, const uint8_t *db, int32_t m, const uint8_t *qy, int32_t n, const int32_t *sub,
							int32_t g, int32_t o, int32_t e, int32_t *vals, struct sa_fit_pay *pays)
{
	int32_t *M = vals, *X = vals + (n + 1), *Y = vals + 2 * (n + 1);
	struct sa_fit_pay *PM = pays, *PX = pays + (n + 1), *PY = pays + 2 * (n + 1);
	for (int32_t c = 0; c <= n; c++) { /* row 0 */
		M[c] = sa_fit_border(method, c, g, o, e);
		X[c] = Y[c] = SA_ID_SCORE_MIN;
		PM[c] = PX[c] = PY[c] = sa_fit_border_row0(c);
	}
	int32_t best = M[n], best_r = 0;
	struct sa_fit_pay best_p = PM[n];
	for (int32_t r = 1; r <= m; r++) {
		const int32_t a = db[r - 1];
		/* column 0 of this row; the values of row r - 1, column c - 1 travel in d* */
		int32_t dM = M[0];
		struct sa_fit_pay dPM = PM[0];
		M[0] = 0;
		X[0] = SA_ID_SCORE_MIN;
		PM[0] = PX[0] = PY[0] = sa_fit_border_col0(r);
		for (int32_t c = 1; c <= n; c++) {
			const int32_t b = qy[c - 1];
			const bool equal = a == b;
			const int32_t upM = M[c], upY = Y[c];
			const struct sa_fit_pay upPM = PM[c], upPY = PY[c];
			int32_t nm;
			struct sa_fit_pay pm;
			if (method == SA_TB_NW) {
				const int32_t match = dM + sub[a * 24 + b], del = upM + g, ins = M[c - 1] + g;
				nm = ins > del ? ins : del;
				nm = nm > match ? nm : match;
				pm = sa_fit_step_nw(sa_tb_encode_nw(nm, match, del), equal, dPM, upPM, PM[c - 1]);
			} else {
				const int32_t sd = dM + sub[b * 24 + a];
				const int32_t xo = M[c - 1] + o, yo = upM + o;
				const int32_t xe = X[c - 1] + e, ye = upY + e;
				const int32_t nx = xo > xe ? xo : xe, ny = yo > ye ? yo : ye;
				nm = nx > sd ? nx : sd;
				nm = ny > nm ? ny : nm;
				const uint32_t rec = sa_tb_encode_affine(false, nm, sd, nx, ny, xo, yo);
				const struct sa_fit_pay px = sa_fit_step_x(rec, PM[c - 1], PX[c - 1]);
				const struct sa_fit_pay py = sa_fit_step_y(rec, upPM, upPY);
				pm = sa_fit_step_m(rec, equal, dPM, px, py);
				X[c] = nx;
				Y[c] = ny;
				PX[c] = px;
				PY[c] = py;
			}
			dM = upM;
			dPM = upPM;
			M[c] = nm;
			PM[c] = pm;
		}
		if (sa_fit_end_before(M[n], r, best, best_r)) { /* (rows arrive in ascending order: strictly greater only) */
			best = M[n];
			best_r = r;
			best_p = PM[n];
		}
	}
	struct sa_fit_result res = { best, best_p.begin, best_r, best_p.identities, best_p.columns };
	return res;
}

#endif /* SA_FIT_CORE_H */
