/* sa_strands_core.h -- the host-compilable part of the two-strand search (sa_strands.hip): the IUPAC complement table, the
 * reverse complement of a store, the geometry of the strand bitmap, the fold rule of one cell, how a row is cut into segments,
 * and fold / strand take done serially.  tests/host_c/strands_test.cpp runs it under ASan / UBSan against a plain loop.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_strand_fold): a strands context holds the M queries followed by their M reverse
 * complements, so every query q has two rows of values, v_fwd = row q and v_rev = row M + q.  Cell (q, d) is REVERSE iff
 * v_rev > v_fwd; equal values keep the forward strand, whatever the raw scores are.  The folded value is the larger one, the
 * folded raw score the raw score of the strand that won.
 *
 * Bitmap: sa_strand_words(N) = (N + 63) / 64 uint64 words per row; bit d & 63 of word d >> 6 of row r is the strand of cell
 * (r, d); bits at or beyond N are zero.
 *
 * Row split: one wave folds one (row, segment), 64 consecutive d per step, so the ballot of a step IS one word of the bitmap.
 * The number of segments is sa_above_segments(N, nq); the bounds are multiples of 64 (whole words dealt evenly), so no word has
 * two writers. */
#ifndef SA_STRANDS_CORE_H
#define SA_STRANDS_CORE_H

#include <stdint.h>
#include <string.h>

#include "../../include/seqalign_hip.h" /* struct sa_input, SA_LUT_SIZE, SA_STRAND_* */
#include "sa_search_above_core.h"       /* sa_above_segments, SA_NB_HD */

/* (SA_STRAND_FORWARD = 0, SA_STRAND_REVERSE = 1, SA_STRAND_NONE = 255 -- an index outside [0, N) -- are the public header's) */

/* ---- complement ---------------------------------------------------------------------------------------------------------- */
/* The upper-case letters of the nucleotide alphabet of the shipped tables, ATGCSWRYKMBVHDN*, and U -> A; every other byte 0:
 * "no complement".  An involution on ATGCSWRYKMBVHDN*. */
static inline void sa_strands_complement_table(uint8_t comp[SA_LUT_SIZE])
{
	static const char from[] = "ATGCSWRYKMBVHDN*U", to[] = "TACGSWYRMKVBDHN*A";
	memset(comp, 0, SA_LUT_SIZE);
	for (int t = 0; from[t]; t++)
		comp[(uint8_t)from[t]] = (uint8_t)to[t];
}

enum { SA_RC_OK = 0, SA_RC_NO_COMPLEMENT = 1, SA_RC_NOT_IN_TABLE = 2 };

/* The first residue of `in` that cannot be reverse-complemented: SA_RC_NO_COMPLEMENT when comp gives 0 for it (or it is not
 * ASCII), SA_RC_NOT_IN_TABLE when lut (may be NULL: not checked) rejects its complement.  *seq / *pos / *byte name it. */
static inline int sa_strands_rc_check(struct sa_input in, const uint8_t *comp, const int32_t *lut, int32_t *seq, int32_t *pos, uint8_t *byte)
{
	for (int32_t k = 0; k < in.num; k++) {
		const uint8_t *s = (const uint8_t *)in.seqs + in.meta[k].off;
		for (int32_t p = 0; p < in.meta[k].len; p++) {
			const uint8_t c = s[p] < SA_LUT_SIZE ? comp[s[p]] : 0;
			const int why = !c ? SA_RC_NO_COMPLEMENT : (lut && (c >= SA_LUT_SIZE || lut[c] < 0)) ? SA_RC_NOT_IN_TABLE : SA_RC_OK;
			if (why != SA_RC_OK) {
				*seq = k;
				*pos = p;
				*byte = s[p];
				return why;
			}
		}
	}
	return SA_RC_OK;
}

/* blob_out[meta[k].off + p] = comp[seqs[meta[k].off + len - 1 - p]], the terminator at meta[k].off + len: the same meta serves.
 * blob_out must not overlap in.seqs.  (sa_strands_rc_check has passed.) */
static inline void sa_strands_rc_write(struct sa_input in, const uint8_t *comp, uint8_t *blob_out)
{
	for (int32_t k = 0; k < in.num; k++) {
		const uint8_t *s = (const uint8_t *)in.seqs + in.meta[k].off;
		uint8_t *o = blob_out + in.meta[k].off;
		const int32_t len = in.meta[k].len;
		for (int32_t p = 0; p < len; p++)
			o[p] = comp[s[len - 1 - p] & (SA_LUT_SIZE - 1)];
		o[len] = 0;
	}
}

/* ---- bitmap and fold ----------------------------------------------------------------------------------------------------- */
static inline SA_NB_HD int64_t sa_strand_words(int64_t n_db) { return (n_db + 63) / 64; }

/* the fold rule of one cell */
static inline SA_NB_HD int sa_strand_pick(int32_t v_fwd, int32_t v_rev) { return v_rev > v_fwd ? SA_STRAND_REVERSE : SA_STRAND_FORWARD; }

/* the strand of cell (., d) of one row of the bitmap; d outside [0, n_db) reads nothing */
static inline SA_NB_HD uint8_t sa_strand_bit(const uint64_t *bits_row, int32_t n_db, int32_t d)
{
	if (d < 0 || d >= n_db)
		return SA_STRAND_NONE;
	return (uint8_t)((bits_row[d >> 6] >> (d & 63)) & 1u);
}

/* segments per row: the rule of sa_above_segments (never more than N / 64, so never more than the words of a row) */
static inline SA_NB_HD int32_t sa_strand_segments(int32_t n_db, int32_t nq) { return sa_above_segments(n_db, nq); }
/* segment s of S covers [begin(s), begin(s + 1)): the words of a row dealt evenly, [0, n_db) once */
static inline SA_NB_HD int32_t sa_strand_seg_begin(int32_t n_db, int32_t S, int32_t s)
{
	const int64_t d = sa_strand_words(n_db) * s / S * 64;
	return (int32_t)(d < n_db ? d : n_db);
}

/* ---- one row, serially, as the kernels do it ----------------------------------------------------------------------------- */
/* fold: segment by segment, word by word.  sfwd / srev / sbest all NULL or all given; vbest may be vfwd and sbest may be sfwd;
 * bits_row (sa_strand_words(n_db) words) may be NULL. */
static inline void sa_strand_fold_row(const int32_t *vfwd, const int32_t *vrev, const int32_t *sfwd, const int32_t *srev, int32_t n_db, int32_t S,
				      int32_t *vbest, int32_t *sbest, uint64_t *bits_row)
{
	for (int32_t s = 0; s < S; s++)
		for (int32_t b = sa_strand_seg_begin(n_db, S, s); b < sa_strand_seg_begin(n_db, S, s + 1); b += 64) {
			uint64_t word = 0;
			for (int32_t d = b; d < b + 64 && d < n_db; d++) {
				const int rev = sa_strand_pick(vfwd[d], vrev[d]);
				word |= (uint64_t)rev << (d - b);
				vbest[d] = rev ? vrev[d] : vfwd[d];
				if (sbest)
					sbest[d] = rev ? srev[d] : sfwd[d];
			}
			if (bits_row)
				bits_row[b >> 6] = word;
		}
}

/* the strands of one row of a hit list at pitch k */
static inline void sa_strand_take_row(const uint64_t *bits_row, int32_t n_db, int32_t k, const int32_t *index_row, uint8_t *strand_row)
{
	for (int32_t t = 0; t < k; t++)
		strand_row[t] = sa_strand_bit(bits_row, n_db, index_row[t]);
}

/* the strands of one row of a CSR: entries [begin, end) of the WHOLE arrays index / strand */
static inline void sa_strand_take_csr_row(const uint64_t *bits_row, int32_t n_db, int64_t begin, int64_t end, const int32_t *index, uint8_t *strand)
{
	for (int64_t e = begin; e < end; e++)
		strand[e] = sa_strand_bit(bits_row, n_db, index[e]);
}

#endif /* SA_STRANDS_CORE_H */
