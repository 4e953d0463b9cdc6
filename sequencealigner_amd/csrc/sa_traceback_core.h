/* sa_traceback_core.h -- what the traceback kernels (sa_traceback.hip) and the host share: the record of a DP cell, where
 * it sits in a pair's scratch area, one step of the walk, the run-length emitter and the mirror for a > b.  Plain C++ that
 * the host compiles as well: tests/host_c/traceback_test.cpp runs it under ASan / UBSan against a literal implementation of
 * the contract over full tables.
 *
 * Contract (include/seqalign_hip.h, "alignments for chosen pairs"), in the canonical orientation: lo = min(a, b) is the row
 * sequence (r = 0 .. m), hi = max(a, b) the column sequence (c = 0 .. n); H / M, X (from the left, consumes a residue of hi)
 * and Y (from above, consumes a residue of lo) are the reference's tables, borders included.
 *
 * RECORD, one byte per computed cell (r >= 1, c >= 1):
 *   bits 0-1  the choice in state M: SA_TB_DIAG, SA_TB_X, SA_TB_Y, SA_TB_STOP (SW: M == 0), tested in that contract order
 *             (stop, diagonal, X, Y)
 *   bit 2     X[r][c] == M[r][c-1] + open  ("X came from open": open wins the tie against extend)
 *   bit 3     Y[r][c] == M[r-1][c] + open
 * NW has one table: its record has both open bits set, so that a gap step always returns to state M, and "X" / "Y" mean one
 * step left / up (up is tested before left).
 *
 * BORDER cells (r == 0 or c == 0) have no record; the walk's move there follows from the border values of nw.c:14-20,
 * ga.c:23-38 and sw.c:18-30 for every scoring a context accepts ((2 max_len + 3) |gap| < 2^30, so no border value meets
 * SCORE_MIN + extend): NW and Gotoh go left along row 0 and up along column 0 until (0, 0); SW stops (M == 0).
 *
 * SCRATCH of a pair, laid out by (strip, step, lane) like the sweep that writes it: strip s holds the columns
 * 64 s + 1 .. 64 s + 64, lane l owns column 64 s + l + 1, step t computes row r = t - l + 1.  Four steps of a lane share
 * one 32-bit word, so the 64 lanes of a wave store 256 contiguous bytes every fourth step:
 *   byte of cell (r, c) = 256 * ((line0(s) + t) / 4) + 4 * l + (t mod 4),   t = r - 1 + l,
 * line0(s) = s * lines(64) and lines(w) = m + w - 1 rounded up to a multiple of four. */
#ifndef SA_TRACEBACK_CORE_H
#define SA_TRACEBACK_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define SA_TB_HD __host__ __device__
#else
#define SA_TB_HD
#endif

enum { SA_TB_DIAG = 0, SA_TB_X = 1, SA_TB_Y = 2, SA_TB_STOP = 3, SA_TB_XOPEN = 4, SA_TB_YOPEN = 8 };
enum { SA_TB_OP_M = 0, SA_TB_OP_I = 1, SA_TB_OP_D = 2 }; /* = the public CIGAR ops: I a residue of a only, D of b only */
enum { SA_TB_STATE_M = 0, SA_TB_STATE_X = 1, SA_TB_STATE_Y = 2 };
enum { SA_TB_NW = 0, SA_TB_GA = 1, SA_TB_SW = 2 }; /* = enum sa_method */

/* ---- encoder: what the fill records for one cell ------------------------------------------------------------------ */

/* NW (nw.c:29-35): h = H[r][c], match = H[r-1][c-1] + S, up = H[r-1][c] + g; anything else came from the left */
static inline SA_TB_HD uint32_t sa_tb_encode_nw(int32_t h, int32_t match, int32_t up)
{
	const uint32_t choice = h == match ? SA_TB_DIAG : h == up ? SA_TB_Y : SA_TB_X;
	return choice | SA_TB_XOPEN | SA_TB_YOPEN;
}

/* Gotoh / SW (ga.c:46-63, sw.c:39-57): m = M[r][c], sd = M[r-1][c-1] + S, x = X[r][c], y = Y[r][c],
 * xopen = M[r][c-1] + open, yopen = M[r-1][c] + open */
static inline SA_TB_HD uint32_t sa_tb_encode_affine(bool sw, int32_t m, int32_t sd, int32_t x, int32_t y, int32_t xopen, int32_t yopen)
{
	const uint32_t choice = (sw && m == 0) ? SA_TB_STOP : m == sd ? SA_TB_DIAG : m == x ? SA_TB_X : SA_TB_Y;
	return choice | (x == xopen ? SA_TB_XOPEN : 0u) | (y == yopen ? SA_TB_YOPEN : 0u);
}

/* SW end cell: does (v, r, c) come before (bv, br, bc) under the key (best descending, r ascending, c ascending)? */
static inline SA_TB_HD bool sa_tb_end_before(int32_t v, int32_t r, int32_t c, int32_t bv, int32_t br, int32_t bc)
{
	return v > bv || (v == bv && (r < br || (r == br && c < bc)));
}

/* ---- scratch geometry --------------------------------------------------------------------------------------------- */

static inline SA_TB_HD int64_t sa_tb_strip_lines(int32_t m, int32_t width) { return ((int64_t)m + width - 1 + 3) & ~(int64_t)3; }

/* bytes of the scratch of a pair with m rows and n columns (a multiple of 256) */
static inline SA_TB_HD int64_t sa_tb_pair_bytes(int32_t m, int32_t n)
{
	const int32_t nstrips = (n + 63) >> 6, last = n - ((nstrips - 1) << 6);
	return 64 * ((int64_t)(nstrips - 1) * sa_tb_strip_lines(m, 64) + sa_tb_strip_lines(m, last));
}

/* byte offset of the record of cell (r, c), 1 <= r <= m, 1 <= c <= n */
static inline SA_TB_HD int64_t sa_tb_cell_offset(int32_t m, int32_t r, int32_t c)
{
	const int32_t s = (c - 1) >> 6, l = (c - 1) & 63;
	const int64_t line = (int64_t)s * sa_tb_strip_lines(m, 64) + (r - 1 + l);
	return 256 * (line >> 2) + 4 * l + (line & 3);
}

/* ---- the walk ------------------------------------------------------------------------------------------------------ */

struct sa_tb_walk {
	int32_t r, c;  /* the cell the walk stands on */
	int32_t state; /* SA_TB_STATE_* */
};

static inline SA_TB_HD bool sa_tb_on_border(const struct sa_tb_walk *w) { return w->r == 0 || w->c == 0; }

/* One step from the cell the walk stands on; `rec` is that cell's record (not read on a border cell).  Returns the op of
 * the column it emits in the canonical orientation (SA_TB_OP_*), or -1: the walk is over and (r, c) is where it stopped. */
static inline SA_TB_HD int sa_tb_step(struct sa_tb_walk *w, int method, uint32_t rec)
{
	if (sa_tb_on_border(w)) {
		if (method == SA_TB_SW || (w->r == 0 && w->c == 0))
			return -1;
		w->state = SA_TB_STATE_M;
		if (w->r == 0) {
			w->c--;
			return SA_TB_OP_D;
		}
		w->r--;
		return SA_TB_OP_I;
	}
	if (w->state == SA_TB_STATE_M) {
		const uint32_t choice = rec & 3u;
		if (choice == SA_TB_STOP)
			return -1;
		if (choice == SA_TB_DIAG) {
			w->r--;
			w->c--;
			return SA_TB_OP_M;
		}
		w->state = (int32_t)choice; /* enter X or Y at this cell */
	}
	if (w->state == SA_TB_STATE_X) {
		w->state = (rec & SA_TB_XOPEN) ? SA_TB_STATE_M : SA_TB_STATE_X;
		w->c--;
		return SA_TB_OP_D;
	}
	w->state = (rec & SA_TB_YOPEN) ? SA_TB_STATE_M : SA_TB_STATE_Y;
	w->r--;
	return SA_TB_OP_I;
}

/* a > b: the caller's a is the column sequence, so a residue of lo only is a residue of b only */
static inline SA_TB_HD int sa_tb_mirror_op(int op, bool flip)
{
	return !flip || op == SA_TB_OP_M ? op : op == SA_TB_OP_I ? SA_TB_OP_D : SA_TB_OP_I;
}

/* ---- run-length emitter -------------------------------------------------------------------------------------------
 * The walk produces the columns end-first: runs are written downwards from `end` (one past the last word of an area of at
 * least m + n words), so they read start-to-end at end - runs.  A run is len << 4 | op. */
struct sa_tb_rle {
	uint32_t *end;
	int32_t runs;
	int32_t op;   /* op of the open run, -1: none */
	uint32_t len;
	int32_t columns;
};

static inline SA_TB_HD void sa_tb_rle_init(struct sa_tb_rle *e, uint32_t *end)
{
	e->end = end;
	e->runs = 0;
	e->op = -1;
	e->len = 0;
	e->columns = 0;
}

/* `write`: this caller owns the store (one lane of the wave on the device) */
static inline SA_TB_HD void sa_tb_rle_flush(struct sa_tb_rle *e, bool write)
{
	if (e->op < 0)
		return;
	e->runs++;
	if (write)
		e->end[-(int64_t)e->runs] = (e->len << 4) | (uint32_t)e->op;
	e->op = -1;
	e->len = 0;
}

static inline SA_TB_HD void sa_tb_rle_push(struct sa_tb_rle *e, int op, bool write)
{
	if (op != e->op) {
		sa_tb_rle_flush(e, write);
		e->op = op;
	}
	e->len++;
	e->columns++;
}

#endif /* SA_TRACEBACK_CORE_H */
