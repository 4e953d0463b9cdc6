/* sa_normalize_core.h -- the contract of the normalised scores (sa_normalize.hip), in a form the host compiles as well:
 * tests/host_c/normalize_test.cpp runs it under ASan / UBSan against __int128 arithmetic.
 *
 * Contract (include/seqalign_hip.h: sa_ctx_normalize): every sequence k has a denominator d[k] -- its self-score under the
 * context's method and scoring, or its length.  The score s of the pair (i, j) becomes, in parts per million (SA_NORM_SCALE),
 *   MIN   floor(s SCALE / min(d[i], d[j]))
 *   MAX   floor(s SCALE / max(d[i], d[j]))
 *   MEAN  floor(2 s SCALE / (d[i] + d[j]))
 * floor rounding towards minus infinity (Python's //, not C's /), saturated to int32; a denominator D <= 0 gives INT32_MIN, the
 * worst score for every consumer.
 *
 * The division: |num| <= 2 * 2^31 * 10^6 < 2^52 and 0 < D < 2^32 are both exact as doubles, so the IEEE quotient is the real
 * quotient rounded once: its floor is the wanted floor or one beside it, and one exact 64-bit multiply-and-compare in each
 * direction settles it.  (|q D| <= |num| + D: no overflow.)  A 64-bit integer division costs the device some 150 instructions; this
 * costs a double division and two multiplies.
 *
 * The walk (sa_norm_column_start, sa_norm_deal): column j of the triangle is the contiguous run packed[j (j - 1) / 2 .. + j), over
 * which d[j] is uniform and d[i] is read in order.  Columns are dealt in pairs (t, N - 1 - t), t < ceil(N / 2): every pair holds
 * N - 1 entries (the middle column of an odd N alone: (N - 1) / 2), so equal shares of pairs are equal shares of work.  The
 * kernel and the serial sa_norm_triangle below walk the same way. */
#ifndef SA_NORMALIZE_CORE_H
#define SA_NORMALIZE_CORE_H

#include <stdint.h>

#include "sa_neighbors_core.h" /* SA_NB_HD */

#define SA_NORM_SRC_SELF 0 /* = SA_NORM_SELF, SA_NORM_LENGTH of include/seqalign_hip.h */
#define SA_NORM_SRC_LENGTH 1
#define SA_NORM_RULE_MIN 0 /* = SA_NORM_MIN, SA_NORM_MAX, SA_NORM_MEAN */
#define SA_NORM_RULE_MAX 1
#define SA_NORM_RULE_MEAN 2
#define SA_NORM_PPM 1000000 /* = SA_NORM_SCALE */

/* floor(num / den) for |num| < 2^52, 0 < den < 2^32 */
static inline SA_NB_HD int64_t sa_norm_floor_div(int64_t num, int64_t den)
{
	int64_t q = (int64_t)((double)num / (double)den); /* (truncates; |q| < 2^52) */
	int64_t r = num - q * den;
	if (r < 0) {
		q -= 1;
		r += den;
	}
	if (r < 0) { /* (the quotient was rounded up across an integer, and truncation then stepped once more) */
		q -= 1;
		r += den;
	}
	if (r >= den) {
		q += 1;
		r -= den;
	}
	if (r >= den)
		q += 1;
	return q;
}

template <int RULE>
static inline SA_NB_HD int32_t sa_norm_value_t(int32_t s, int32_t di, int32_t dj)
{
	int64_t den, num = (int64_t)s * SA_NORM_PPM;
	if (RULE == SA_NORM_RULE_MIN)
		den = di < dj ? di : dj;
	else if (RULE == SA_NORM_RULE_MAX)
		den = di > dj ? di : dj;
	else {
		den = (int64_t)di + dj;
		num *= 2;
	}
	if (den <= 0)
		return INT32_MIN;
	const int64_t q = sa_norm_floor_div(num, den);
	return q < INT32_MIN ? INT32_MIN : q > INT32_MAX ? INT32_MAX : (int32_t)q;
}

/* any other rule: treated as MEAN (the entry points refuse it before this is reached) */
static inline SA_NB_HD int32_t sa_norm_value_rule(int32_t s, int32_t di, int32_t dj, int32_t rule)
{
	return rule == SA_NORM_RULE_MIN   ? sa_norm_value_t<SA_NORM_RULE_MIN>(s, di, dj)
	       : rule == SA_NORM_RULE_MAX ? sa_norm_value_t<SA_NORM_RULE_MAX>(s, di, dj)
					  : sa_norm_value_t<SA_NORM_RULE_MEAN>(s, di, dj);
}

/* first packed index of column j; 64-bit: it passes 2^32 at N = 92 683 */
static inline SA_NB_HD int64_t sa_norm_column_start(int64_t j) { return j * (j - 1) / 2; }
/* units of the deal: t = 0 .. sa_norm_units(N) - 1 */
static inline SA_NB_HD int64_t sa_norm_units(int64_t num) { return (num + 1) / 2; }
/* the columns of unit t: *a = t and *b = N - 1 - t; *b = -1 when they coincide (the middle column of an odd N) */
static inline SA_NB_HD void sa_norm_deal(int64_t num, int64_t t, int64_t *a, int64_t *b)
{
	*a = t;
	*b = num - 1 - t == t ? -1 : num - 1 - t;
}

/* the whole triangle, serially, by the kernel's walk (host tests; in == out is allowed) */
static inline void sa_norm_triangle(const int32_t *in, const int32_t *den, int32_t num, int32_t rule, int32_t *out)
{
	for (int64_t t = 0; t < sa_norm_units(num); t++) {
		int64_t col[2];
		sa_norm_deal(num, t, &col[0], &col[1]);
		for (int c = 0; c < 2; c++) {
			const int64_t j = col[c];
			if (j < 0)
				continue;
			const int64_t base = sa_norm_column_start(j);
			for (int64_t i = 0; i < j; i++)
				out[base + i] = sa_norm_value_rule(in[base + i], den[i], den[j], rule);
		}
	}
}

#endif /* SA_NORMALIZE_CORE_H */
