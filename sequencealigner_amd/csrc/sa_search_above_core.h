/* sa_search_above_core.h -- the host-compilable part of the threshold search (sa_search_above.hip): how a row of the rectangle
 * is cut into segments, the size of the scratch, and count / scan / fill done serially.  tests/host_c/search_above_test.cpp
 * runs it under ASan / UBSan against a plain loop.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_hits_above_offsets): database sequence d is a hit of row r iff
 * vrect[r * N + d] >= min_value (sa_edge_pass of sa_edges_core.h).  The result is a CSR over the rows: offsets int64[nq + 1]
 * (offsets[0] = 0), index / value / score int32[offsets[nq]], row r's hits in ASCENDING d.
 *
 * Row split: one wave scans one (row, segment), as in sa_k_hits_part.  A segment leaves no list behind, only a count, so what
 * bounds S is the wave step alone: S = 1 when the rows fill the device by themselves (SA_HITS_ROWS_FILL); otherwise nq * S is
 * about SA_HITS_WAVES, held to N / 64 so that a segment is at least one step of 64 candidates long.  S depends on (N, nq)
 * only -- never on the device -- so the scratch size is known without one.  The bounds are those of sa_hits_seg_begin: not
 * multiples of 64 in general.
 *
 * Scratch: nq * S + 1 int64.  The count pass leaves the hits of (row r, segment s) at [r * S + s]; the scan turns them into the
 * exclusive sums in place and puts the total at [nq * S].  Segments are numbered row by row, and inside a row by ascending d,
 * so the scanned entry IS where the segment's first hit goes: nothing depends on which wave arrives first. */
#ifndef SA_SEARCH_ABOVE_CORE_H
#define SA_SEARCH_ABOVE_CORE_H

#include <stdint.h>

#include "sa_edges_core.h"  /* sa_edge_pass */
#include "sa_search_core.h" /* SA_HITS_WAVES, SA_HITS_ROWS_FILL, sa_hits_seg_begin */

#define SA_ABOVE_STEP 64 /* candidates of one wave step: a segment is never shorter (unless the row is) */

/* segments per row */
static inline SA_NB_HD int32_t sa_above_segments(int32_t n_db, int32_t nq)
{
	if (nq >= SA_HITS_ROWS_FILL)
		return 1;
	int64_t s = (SA_HITS_WAVES + (int64_t)nq - 1) / nq;
	const int64_t cap = n_db / SA_ABOVE_STEP;
	if (s > cap)
		s = cap;
	return (int32_t)(s < 1 ? 1 : s);
}

/* int64 entries of the scratch: one per (row, segment) and the total */
static inline SA_NB_HD int64_t sa_above_scratch_elems(int32_t n_db, int32_t nq) { return (int64_t)nq * sa_above_segments(n_db, nq) + 1; }

/* ---- one row, serially, as the kernels do it ----------------------------------------------------------------------------- */
/* count: the hits of every segment of one row into counts[0 .. S) */
static inline void sa_above_count_row(const int32_t *vrow, int32_t n_db, int32_t S, int32_t min_value, int64_t *counts)
{
	for (int32_t s = 0; s < S; s++) {
		int64_t c = 0;
		for (int32_t d = sa_hits_seg_begin(n_db, S, s); d < sa_hits_seg_begin(n_db, S, s + 1); d++)
			c += sa_edge_pass(vrow[d], min_value);
		counts[s] = c;
	}
}

/* scan: counts[0 .. n) become their exclusive sums in place, counts[n] the total */
static inline void sa_above_scan(int64_t *counts, int64_t n)
{
	int64_t sum = 0;
	for (int64_t t = 0; t < n; t++) {
		const int64_t c = counts[t];
		counts[t] = sum;
		sum += c;
	}
	counts[n] = sum;
}

/* offsets[0 .. nq] from the scanned scratch */
static inline void sa_above_offsets(const int64_t *scanned, int32_t nq, int32_t S, int64_t *offsets)
{
	for (int32_t r = 0; r < nq; r++)
		offsets[r] = scanned[(int64_t)r * S];
	offsets[nq] = scanned[(int64_t)nq * S];
}

/* fill: the segments of one row, each from its own scanned base (bases = scanned + r * S), never at or beyond `end`
 * (= offsets[r + 1]).  index / value / score are the WHOLE arrays; value and score may be NULL; srow (the raw scores of the
 * row) is read at the hits only, and only when score is not NULL. */
static inline void sa_above_fill_row(const int32_t *vrow, const int32_t *srow, int32_t n_db, int32_t S, int32_t min_value, const int64_t *bases,
				     int64_t end, int32_t *index, int32_t *value, int32_t *score)
{
	for (int32_t s = 0; s < S; s++) {
		int64_t at = bases[s];
		for (int32_t d = sa_hits_seg_begin(n_db, S, s); d < sa_hits_seg_begin(n_db, S, s + 1); d++) {
			const int32_t v = vrow[d];
			if (!sa_edge_pass(v, min_value))
				continue;
			if (at < end) {
				index[at] = d;
				if (value)
					value[at] = v;
				if (score)
					score[at] = srow[d];
			}
			at++;
		}
	}
}

#endif /* SA_SEARCH_ABOVE_CORE_H */
