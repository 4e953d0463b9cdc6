/* sa_search_quantity_core.h -- the host-compilable part of the search quantities (sa_search_quantity.hip): how the rectangle
 * sweep cuts rows into pieces and a piece into head / 16-byte vectors / tail, which pair a wave item of the rectangle form of
 * the identity sweep is, and the sweep and the take gather done serially.  tests/host_c/search_quantity_test.cpp runs it under
 * ASan / UBSan.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_normalize_rect): row r of a rectangle of pitch N is query q0 + r; the pair of
 * element (r, d) is (d, N + q0 + r) of the concatenated store -- d the row sequence -- so its value is
 * sa_norm_value(rect[r * N + d], den[d], den[N + q0 + r], rule).  The rule itself is sa_normalize_core.h's; there is no second one.
 *
 * The walk: a row is cut into pieces of SA_SQ_PIECE consecutive elements exactly as sa_k_rect_rows cuts it (piece p is row
 * p / per_row, elements [(p % per_row) * SA_SQ_PIECE, ...)); over a piece the query's denominator is uniform and the database
 * denominators are read in order.  A row begins at byte 4 r N, any alignment: the up to three elements before the first 16-byte
 * boundary of the piece and after the last go one by one, the body as 16-byte vectors -- one per thread of a workgroup of
 * SA_SQ_PIECE / 4 threads.  When source and destination disagree about where that boundary is, the whole piece goes element by
 * element.  Every element offset is 64-bit: a batch's rectangle may pass 2^31 elements. */
#ifndef SA_SEARCH_QUANTITY_CORE_H
#define SA_SEARCH_QUANTITY_CORE_H

#include <stdint.h>

#include "sa_normalize_core.h"

#define SA_SQ_PIECE 1024 /* elements of a piece: the piece of sa_k_rect_rows (four per thread of a 256-thread workgroup) */

static inline SA_NB_HD int64_t sa_sq_pieces_per_row(int64_t n_db) { return (n_db + SA_SQ_PIECE - 1) / SA_SQ_PIECE; }
static inline SA_NB_HD int64_t sa_sq_pieces(int64_t n_db, int64_t nq) { return sa_sq_pieces_per_row(n_db) * nq; }
/* piece p: row *r, elements [*d0, *d0 + *len) of it; 1 <= *len <= SA_SQ_PIECE */
static inline SA_NB_HD void sa_sq_piece(int64_t n_db, int64_t p, int64_t *r, int64_t *d0, int32_t *len)
{
	const int64_t per_row = sa_sq_pieces_per_row(n_db);
	*r = p / per_row;
	*d0 = (p - *r * per_row) * SA_SQ_PIECE;
	*len = (int32_t)(n_db - *d0 < SA_SQ_PIECE ? n_db - *d0 : SA_SQ_PIECE);
}
/* element offset of (row r, database sequence d) in a rectangle of pitch n_db */
static inline SA_NB_HD int64_t sa_sq_at(int64_t n_db, int64_t r, int64_t d) { return r * n_db + d; }

/* a piece of `len` elements that begins at byte addresses in / out: *head elements one by one, then *vecs 16-byte vectors, then
 * the tail len - *head - 4 * *vecs one by one (head, tail <= 3 unless the two addresses disagree modulo 16: then head = len) */
static inline SA_NB_HD void sa_sq_split(uint64_t in, uint64_t out, int32_t len, int32_t *head, int32_t *vecs)
{
	int32_t h = (int32_t)(((16 - (in & 15)) & 15) / 4);
	if (((in ^ out) & 15) != 0 || h > len)
		h = len;
	*head = h;
	*vecs = (len - h) / 4;
}

/* wave item w of the rectangle form of the identity sweep over queries [q0, ...): element w of the dense outputs, the pair
 * (*i, *j) = (d, N + q0 + r) with w = r * N + d */
static inline SA_NB_HD void sa_sq_identity_item(int32_t n_db, int32_t q0, int64_t w, int32_t *i, int32_t *j)
{
	const int64_t r = w / n_db;
	*i = (int32_t)(w - r * n_db);
	*j = (int32_t)(n_db + q0 + r);
}

/* one hit of the take gather: INT32_MIN for an index outside [0, N) (the caller's error; nothing outside the rectangle is read) */
static inline SA_NB_HD int32_t sa_sq_take_one(const int32_t *rect, int32_t n_db, int32_t k, const int32_t *index, int64_t t)
{
	const int64_t r = t / k;
	const int32_t d = index[t];
	return d >= 0 && d < n_db ? rect[sa_sq_at(n_db, r, d)] : INT32_MIN;
}

/* rows [0, nq) serially, by the kernel's walk: thread `tid` of a piece does what it does on the device (host tests; in == out is
 * allowed).  `in` and `out` point at element 0 of row 0. */
static inline void sa_sq_normalize_rect(const int32_t *in, int32_t n_db, int32_t q0, int32_t nq, const int32_t *den, int32_t rule, int32_t *out)
{
	for (int64_t p = 0; p < sa_sq_pieces(n_db, nq); p++) {
		int64_t r, d0;
		int32_t len, head, vecs;
		sa_sq_piece(n_db, p, &r, &d0, &len);
		const int64_t at = sa_sq_at(n_db, r, d0);
		const int32_t dq = den[n_db + q0 + r];
		sa_sq_split((uint64_t)(uintptr_t)(in + at), (uint64_t)(uintptr_t)(out + at), len, &head, &vecs);
		for (int32_t tid = 0; tid < SA_SQ_PIECE / 4; tid++) {
			for (int32_t e = tid; e < head; e += SA_SQ_PIECE / 4)
				out[at + e] = sa_norm_value_rule(in[at + e], den[d0 + e], dq, rule);
			if (tid < vecs)
				for (int u = 0; u < 4; u++) {
					const int32_t e = head + 4 * tid + u;
					out[at + e] = sa_norm_value_rule(in[at + e], den[d0 + e], dq, rule);
				}
			const int32_t e = head + 4 * vecs + tid;
			if (e < len)
				out[at + e] = sa_norm_value_rule(in[at + e], den[d0 + e], dq, rule);
		}
	}
}

static inline void sa_sq_take(const int32_t *rect, int32_t n_db, int32_t nq, int32_t k, const int32_t *index, int32_t *out)
{
	for (int64_t t = 0; t < (int64_t)nq * k; t++)
		out[t] = sa_sq_take_one(rect, n_db, k, index, t);
}

#endif /* SA_SEARCH_QUANTITY_CORE_H */
