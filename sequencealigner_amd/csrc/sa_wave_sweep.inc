/*
 * sa_wave_sweep.inc -- the anti-diagonal s32 score sweep of one pair by one wavefront (gfx950, wave64): text that
 * sa_k_pair_per_wave (sa_generic.hip) and sa_k_self (sa_normalize.hip) include inside their loops, after sa_wave_sweep.h.
 * It is text and not a function on purpose: inlined from a function of its own, the same statements reach the code generator
 * with the row-range test of a step in its negated form, which puts one more scalar instruction in front of the residue load
 * of every step (sa_k_pair_per_wave<nw>: + 3.6 % of its time).
 *
 * The always-applicable path: exact s32 restatement of the reference recurrences
 *   NW  src/bio/method/nw.c:14-41      GA  src/bio/method/ga.c:23-67      SW  src/bio/method/sw.c:18-61
 * with no assumption on gap values or sequence length.  Lane l owns column c = 64 * strip + l + 1 of the DP matrix (the
 * column sequence), rows enter at lane 0 and travel one lane per step, so step t of a strip computes its anti-diagonal t.
 * The left / diagonal dependency crosses lanes with a wave shift; the strip's last column is parked in the wave's boundary
 * lines (the context's scratch: max_len + 2 ints each for M and X) so that the next 64-column strip continues from it.
 *
 * Reads, by these names, from the kernel:
 *   METHOD                the kernel's template parameter
 *   s_sub                 the 24 x 24 table in LDS
 *   bndM, bndX            this wave's boundary lines
 *   g, o, e               gap (NW); open, extend (GA, SW)
 *   lane                  threadIdx.x & 63
 *   ci, m / cj, n         codes and length of the row / the column sequence
 * Defines `mn` = M[m][n] in every lane and `best`, this lane's SW running maximum.
 */
/* closed forms of the reference's iteratively filled borders:
 * NW nw.c:16-20: k*g.  GA ga.c:26-38: B(1) = max(0+o, SCORE_MIN+e), B(k) = B(k-1)+max(o,e). */
const int32_t ga_b1 = imax(o, SCORE_MIN + e);
const int32_t ga_w = imax(o, e);
auto border = [&](int32_t k) -> int32_t {
	if (METHOD == SA_METHOD_NW)
		return k * g;
	if (METHOD == SA_METHOD_GA)
		return k == 0 ? 0 : ga_b1 + (k - 1) * ga_w;
	return 0;
};
const int32_t nstrips = (n + 63) >> 6;
int32_t best = 0; /* SW running maximum, sw.c:33,57 */
int32_t h = 0;

for (int32_t s = 0; s < nstrips; s++) {
	const int32_t c = (s << 6) + lane + 1;
	const bool colvalid = c <= n;
	const int32_t b = colvalid ? cj[c - 1] : 0;
	const int32_t width = (n - (s << 6)) < 64 ? (n - (s << 6)) : 64;
	const bool last_strip = s + 1 == nstrips;
	h = border(c);                /* M[0][c]                                   */
	int32_t y = SCORE_MIN;        /* gap_y[0][c]          ga.c:29, sw.c:22     */
	int32_t x = SCORE_MIN;        /* gap_x[r][c] of the row just computed      */
	int32_t diag = border(c - 1); /* M[0][c-1] until the first row arrives     */
	const int32_t steps = m + width - 1;

	for (int32_t t = 0; t < steps; t++) {
		const int32_t r = t - lane + 1;
		int32_t lm = from_left(h);
		int32_t lx = SCORE_MIN;
		if (METHOD != SA_METHOD_NW)
			lx = from_left(x);
		if (lane == 0) {
			if (s == 0) {
				lm = border(r); /* M[r][0]   nw.c:19, ga.c:32-37, sw.c:26-29 */
				lx = SCORE_MIN; /* gap_x[r][0]                               */
			} else if (r <= m) { /* (r >= 1 in lane 0; the lines hold max_len + 2 ints) */
				lm = bndM[r];
				if (METHOD != SA_METHOD_NW)
					lx = bndX[r];
			}
		}
		const bool valid = colvalid && r >= 1 && r <= m;
		const int32_t a = valid ? ci[r - 1] : 0;
		int32_t nm, nx = SCORE_MIN, ny = SCORE_MIN;
		if (METHOD == SA_METHOD_NW) {
			/* nw.c:29-35: [code of row][code of column] */
			const int32_t match = diag + s_sub[a * SA_SUB_DIM + b];
			const int32_t del = h + g;
			const int32_t ins = lm + g;
			nm = imax(ins, imax(del, match));
		} else {
			/* ga.c:46-63 / sw.c:39-57: [code of column][code of row] */
			const int32_t sd = diag + s_sub[b * SA_SUB_DIM + a];
			nx = imax(lm + o, lx + e);
			ny = imax(h + o, y + e);
			nm = (METHOD == SA_METHOD_SW) ? imax(sd, 0) : sd;
			nm = imax(nx, nm);
			nm = imax(ny, nm);
		}
		diag = lm;
		if (valid) {
			h = nm;
			x = nx;
			y = ny;
			if (METHOD == SA_METHOD_SW)
				best = imax(best, nm);
			if (lane == 63 && !last_strip) {
				bndM[r] = nm;
				if (METHOD != SA_METHOD_NW)
					bndX[r] = nx;
			}
		}
	}
	if (!last_strip)
		__threadfence_block(); /* boundary column visible to this wave's next strip */
}
const int32_t mn = __shfl(h, (n - 1) & 63, 64); /* M[m][n] sits in the lane owning column n */
