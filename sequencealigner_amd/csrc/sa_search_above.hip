/*
 * sa_search_above.hip -- every hit of a search at or above a threshold, as a CSR over the rows of the M x N rectangle of a
 * search context (sa_ctx_hits_above_offsets, sa_ctx_hits_above_fill, sa_hip_search_above).  No reference counterpart.  The
 * contract is in include/seqalign_hip.h, the segment rule and the serial restatement in sa_search_above_core.h, which the host
 * compiles as well.
 *
 * The answer has no fixed length per row, so it is built as the score graph is (sa_edges.hip): count, scan, fill, no atomics.
 * What differs is the sweep: a row of the rectangle is contiguous, and with three queries and a million database sequences one
 * wave per row is three waves.  So every row is cut into S segments (sa_above_segments) and one wave scans one (row, segment),
 * 64 candidates per step as in the sweep of sa_k_hits_part, the steps in groups of AB_DEPTH: the loads of the next group are in
 * flight while this one is scanned.
 *   count   sa_k_above<false>: the population count of the ballot of the pass predicate, summed over the steps, goes to
 *           scratch[r * S + seg].
 *   scan    sa_k_above_scan: one workgroup turns the nq * S counts into their exclusive sums in place (the scheme of
 *           sa_k_edge_scan), the total behind them; then offsets[r] = scratch[r * S], offsets[nq] = the total.
 *   fill    sa_k_above<true>: the same sweep from the segment's scanned base.  Steps come in ascending order and lanes are
 *           ascending d, so a passing lane's place is base + the hits of the steps before + the passing lanes below it
 *           (ballot + mbcnt): ascending d without a sort, and the same bytes whatever the timing.  Only passing lanes read the
 *           raw-score rectangle.
 * Every element offset is 64-bit: nq * N may pass 2^31.
 */
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "sa_ctx.h"
#include "sa_search_above_core.h"
#include "sa_strands_core.h"

struct sa_hitlist {
	int32_t queries = 0;
	int64_t count = 0;
	int64_t *offsets = nullptr; /* queries + 1 */
	int32_t *index = nullptr;   /* count (room for one element when count == 0: never a null pointer for a valid result) */
	int32_t *value = nullptr;
	int32_t *score = nullptr; /* raw scores asked for: the same array as value */
	uint8_t *strand = nullptr; /* sa_hip_search_above_strands only */
	~sa_hitlist()
	{
		free(offsets);
		free(index);
		free(strand);
		if (score != value)
			free(score);
		free(value);
	}
};

namespace {

constexpr int AB_THREADS = 256; /* four waves */
/* Steps of 64 candidates a wave keeps in flight: it scans a group of AB_DEPTH steps while the loads of the next group are on their
 * way.  One step ahead leaves 256 bytes per wave in flight, 8 KiB per CU at eight waves per SIMD, and the count pass at a quarter
 * of the HBM roof; four steps make it 32 KiB per CU. */
constexpr int AB_DEPTH = 4;

/* passing lanes below this one */
__device__ __forceinline__ int ab_below(uint64_t pass)
{
	return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(pass >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pass, 0u));
}

/* Wave w of the grid scans segment w % S of row w / S.  FILL = false: scratch[w] = the hits of the segment (scratch is
 * written).  FILL = true: scratch and offsets are read, index / value / score are written; a row never writes at or beyond
 * offsets[r + 1], whatever the caller handed in.  (No __restrict__ on vrect / rect: they may be the same rectangle.) */
template <bool FILL>
__global__ __launch_bounds__(AB_THREADS) void sa_k_above(const int32_t *vrect, const int32_t *rect, int32_t n_db, int32_t nq, int32_t S,
							  int32_t min_value, int64_t *scratch, const int64_t *__restrict__ offsets,
							  int32_t *__restrict__ index, int32_t *__restrict__ value, int32_t *__restrict__ score)
{
	const int lane = threadIdx.x & 63;
	const int64_t w = (int64_t)blockIdx.x * (AB_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (w >= (int64_t)nq * S) /* (wave-uniform) */
		return;
	const int64_t r = w / S;
	const int32_t seg = (int32_t)(w - r * S);
	const int32_t c0 = sa_hits_seg_begin(n_db, S, seg), c1 = sa_hits_seg_begin(n_db, S, seg + 1);
	const int64_t row_at = r * (int64_t)n_db;
	const int32_t *row = vrect + row_at;
	int64_t cursor = FILL ? scratch[w] : 0; /* (wave-uniform) count: the hits so far; fill: the next free place */
	const int64_t end = FILL ? offsets[r + 1] : 0;
	int64_t c = (int64_t)c0 + lane; /* (64-bit: c1 + a group may pass INT32_MAX) */
	int32_t v[AB_DEPTH], vn[AB_DEPTH];
#pragma unroll
	for (int u = 0; u < AB_DEPTH; u++)
		v[u] = c + u * SA_ABOVE_STEP < c1 ? row[c + u * SA_ABOVE_STEP] : 0;
	for (int64_t b = c0; b < c1; b += AB_DEPTH * SA_ABOVE_STEP) {
		const int64_t cn = c + AB_DEPTH * SA_ABOVE_STEP;
#pragma unroll
		for (int u = 0; u < AB_DEPTH; u++) /* the next group: in flight while this one is scanned */
			vn[u] = cn + u * SA_ABOVE_STEP < c1 ? row[cn + u * SA_ABOVE_STEP] : 0;
#pragma unroll
		for (int u = 0; u < AB_DEPTH; u++) { /* the steps of the group, in ascending d */
			const int64_t cu = c + u * SA_ABOVE_STEP;
			const bool mine = cu < c1 && sa_edge_pass(v[u], min_value);
			const uint64_t pass = __ballot(mine);
			if (FILL) {
				const int64_t at = cursor + ab_below(pass);
				if (mine && at < end) {
					index[at] = (int32_t)cu;
					if (value)
						value[at] = v[u];
					if (score)
						score[at] = rect[row_at + cu];
				}
			}
			cursor += __popcll(pass);
		}
		c = cn;
#pragma unroll
		for (int u = 0; u < AB_DEPTH; u++)
			v[u] = vn[u];
	}
	if (!FILL && lane == 0)
		scratch[w] = cursor;
}

/* One workgroup: scratch[0 .. count) hold the hits of the (row, segment)s; afterwards they hold the exclusive sums and
 * scratch[count] the total.  In place: every thread reads its element before the tile's barrier and writes it after.  Then
 * offsets[r] = scratch[r * S] and offsets[nq] = the total (the workgroup's own writes, behind a barrier). */
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void sa_k_above_scan(int64_t *__restrict__ scratch, int32_t nq, int32_t S, int64_t *__restrict__ offsets)
{
	__shared__ int64_t wave_sum[SCAN_THREADS / 64];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t count = (int64_t)nq * S;
	int64_t carry = 0; /* the sum of every tile before this one (the same in every thread) */
	for (int64_t base = 0; base < count; base += SCAN_THREADS) {
		const int64_t t = base + tid;
		const int64_t own = t < count ? scratch[t] : 0;
		int64_t v = own;
#pragma unroll
		for (int d = 1; d < 64; d *= 2) { /* inclusive scan of the wave */
			const int64_t up = __shfl_up(v, d, 64);
			if (lane >= d)
				v += up;
		}
		if (lane == 63)
			wave_sum[wave] = v;
		__syncthreads();
		int64_t before = 0, tile = 0;
#pragma unroll
		for (int w = 0; w < SCAN_THREADS / 64; w++) {
			const int64_t s = wave_sum[w];
			before += w < wave ? s : 0;
			tile += s;
		}
		if (t < count)
			scratch[t] = carry + before + v - own;
		carry += tile;
		__syncthreads();
	}
	if (tid == 0) {
		scratch[count] = carry;
		offsets[nq] = carry;
	}
	__threadfence_block();
	__syncthreads();
	for (int64_t r = tid; r < nq; r += SCAN_THREADS)
		offsets[r] = scratch[r * S];
}

std::atomic<double> g_last_above_seconds{ 0.0 };

int offsets_launch(const int32_t *d_vrect, int32_t n_db, int32_t nq, int32_t min_value, int64_t *d_offsets, int64_t *d_scratch, hipStream_t s)
{
	const int32_t S = sa_above_segments(n_db, nq);
	constexpr int WPB = AB_THREADS / 64;
	const int64_t waves = (int64_t)nq * S;
	hipLaunchKernelGGL(sa_k_above<false>, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(AB_THREADS), 0, s, d_vrect, (const int32_t *)nullptr, n_db,
			   nq, S, min_value, d_scratch, (const int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	hipLaunchKernelGGL(sa_k_above_scan, dim3(1), dim3(SCAN_THREADS), 0, s, d_scratch, nq, S, d_offsets);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

int fill_launch(const int32_t *d_vrect, const int32_t *d_rect, int32_t n_db, int32_t nq, int32_t min_value, const int64_t *d_offsets,
		const int64_t *d_scratch, int32_t *d_index, int32_t *d_value, int32_t *d_score, hipStream_t s)
{
	const int32_t S = sa_above_segments(n_db, nq);
	constexpr int WPB = AB_THREADS / 64;
	const int64_t waves = (int64_t)nq * S;
	hipLaunchKernelGGL(sa_k_above<true>, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(AB_THREADS), 0, s, d_vrect, d_rect, n_db, nq, S, min_value,
			   const_cast<int64_t *>(d_scratch), d_offsets, d_index, d_value, d_score);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

/* what the two device-resident calls refuse alike */
bool above_check(const char *who, const sa_ctx *ctx, int32_t nq, const void *d_scratch)
{
	if (nq < 1 || nq > ctx->search_queries) {
		sa_set_error("%s: %d rows, the context has %d queries: nq must be in [1, %d]", who, nq, ctx->search_queries, ctx->search_queries);
		return false;
	}
	if (reinterpret_cast<uintptr_t>(d_scratch) % alignof(int64_t)) { /* (the counts are 64-bit) */
		sa_set_error("%s: scratch not 8-byte aligned", who);
		return false;
	}
	return true;
}

struct DevBuf {
	void *p = nullptr;
	size_t bytes = 0;
	~DevBuf() { (void)hipFree(p); }
	bool alloc(const char *who, size_t want, const char *what)
	{
		if (hipMalloc(&p, std::max<size_t>(want, 8)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			sa_set_error("%s: %s (%.2f GiB) does not fit the device's memory", who, what, (double)want / (double)(1 << 30));
			return false;
		}
		bytes = want;
		return true;
	}
};

/* host arrays that grow with the batches */
bool grow(int32_t **p, size_t elems)
{
	void *q = realloc(*p, sizeof(int32_t) * std::max<size_t>(elems, 1));
	if (!q)
		return false;
	*p = static_cast<int32_t *>(q);
	return true;
}

bool grow8(uint8_t **p, size_t elems)
{
	void *q = realloc(*p, std::max<size_t>(elems, 1));
	if (!q)
		return false;
	*p = static_cast<uint8_t *>(q);
	return true;
}

/* norm != NULL: normalised scores; pid_denom != NULL: percent identity; neither: raw scores.  strands: sa_hip_search_above_strands
 * -- both strands of every query (the reverse complements under comp_in; NULL: sa_dna_complement's), folded before the count */
sa_hitlist *above_impl(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t min_value, const struct sa_norm *norm,
		       const int32_t *pid_denom, bool strands = false, const uint8_t *comp_in = nullptr)
{
	const char *who = strands ? "sa_hip_search_above_strands" : "sa_hip_search_above";
	if (!sc) {
		sa_set_error("%s: null argument", who);
		return nullptr;
	}
	if (norm && pid_denom) {
		sa_set_error("%s: norm and pid_denom exclude each other", who);
		return nullptr;
	}
	if (db.num < 1 || queries.num < 1) {
		sa_set_error("%s: empty store (%d database sequences, %d queries; min: 1 each)", who, db.num, queries.num);
		return nullptr;
	}
	if (!db.seqs || !db.meta || !queries.seqs || !queries.meta) {
		sa_set_error("%s: null sequence store", who);
		return nullptr;
	}
	if (norm && !sa_norm_check(who, norm))
		return nullptr;
	if (pid_denom && !sa_identity_denom_check(who, *pid_denom))
		return nullptr;
	uint8_t dna[SA_LUT_SIZE];
	sa_strands_complement_table(dna);
	const uint8_t *comp = comp_in ? comp_in : dna;
	if (strands && !sa_strands_inputs_check(who, db, queries, sc, comp))
		return nullptr;
	if (sa_hip_device_count() <= 0) {
		sa_set_error("No HIP devices available; libseqalign_hip has no CPU fallback");
		return nullptr;
	}
	struct Ctx {
		sa_ctx *c = nullptr;
		~Ctx() { sa_ctx_destroy(c); }
	} cx;
	cx.c = strands ? sa_ctx_create_search_strands(0, db, queries, sc, comp) : sa_ctx_create_search(0, db, queries, sc);
	if (!cx.c)
		return nullptr;
	sa_ctx *ctx = cx.c;
	const int64_t n = db.num, m = queries.num, words = sa_strand_words(n);
	const bool quantity = norm || pid_denom, aligned = !pid_denom;
	/* Batch: as sa_hip_search_norm / _pid size it, with the scratch of this call in place of the hit lists.  Per query: the
	 * range row (the longest, N + M - 1 elements; none under percent identity), a row of each rectangle (raw scores: the one),
	 * and 8 bytes of scratch -- the entries of a batch are at most SA_HITS_WAVES + nq + 1, the rest is inside the quarter left
	 * free.  The hits themselves are sized once they are counted. */
	if (pid_denom && !sa_identity_payload_scratch(ctx))
		return nullptr;
	size_t free_b = 0, total_b = 0;
	SA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b), return nullptr);
	/* Both strands: the range row is N + 2 M - 1 elements at most (the two halves use the one buffer in turn), every rectangle has a
	 * reverse twin, and a row of the strand bitmap is added. */
	const int64_t per_query = strands ? (aligned ? 4 * (n + 2 * m) : 0) + (quantity ? 16 : 8) * n + 8 * words + 8
					  : (aligned ? 4 * (n + m) : 0) + (quantity ? 8 : 4) * n + 8;
	int64_t budget = (int64_t)(free_b - free_b / 4);
	if (ctx->env.search_batch_bytes > 0)
		budget = std::min<int64_t>(budget, ctx->env.search_batch_bytes);
	const int32_t nqb = (int32_t)std::max<int64_t>(1, std::min<int64_t>(m, budget / per_query));
	size_t range_bytes = 0, scratch_bytes = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = (int32_t)std::min<int64_t>(nqb, m - q0);
		if (aligned)
			range_bytes = std::max(range_bytes, sa_search_scratch_bytes(ctx, (int32_t)(strands ? m + q0 : q0), nq));
		scratch_bytes = std::max(scratch_bytes, sizeof(int64_t) * (size_t)sa_above_scratch_elems((int32_t)n, nq));
	}
	DevBuf d_range, d_rect, d_vrect, d_den, d_scratch, d_offsets, d_out, d_rrev, d_vrev, d_bits;
	const size_t dens = (size_t)(strands ? n + 2 * m : n + m);
	if ((aligned && !d_range.alloc(who, range_bytes, "the packed range of a query batch")) ||
	    (norm && !d_den.alloc(who, sizeof(int32_t) * dens, "the denominators")) ||
	    (strands && (!d_rrev.alloc(who, sizeof(int32_t) * (size_t)nqb * (size_t)n, "the reverse rectangle of a query batch") ||
			 (quantity && !d_vrev.alloc(who, sizeof(int32_t) * (size_t)nqb * (size_t)n, "the reverse value rectangle of a query batch")) ||
			 !d_bits.alloc(who, sizeof(uint64_t) * (size_t)nqb * (size_t)words, "the strand bitmap of a query batch"))) ||
	    !d_rect.alloc(who, sizeof(int32_t) * (size_t)nqb * (size_t)n, "the rectangle of a query batch") ||
	    (quantity && !d_vrect.alloc(who, sizeof(int32_t) * (size_t)nqb * (size_t)n, "the value rectangle of a query batch")) ||
	    !d_scratch.alloc(who, scratch_bytes, "the segment counts") ||
	    !d_offsets.alloc(who, sizeof(int64_t) * ((size_t)nqb + 1), "the offsets of a query batch"))
		return nullptr;
	struct Sync { /* the stream is drained before the buffers above are freed (declared after them) */
		hipStream_t s = nullptr;
		hipEvent_t ev[7] = {}; /* start, range aligned, rows moved, values done, counted + scanned, fill begins, filled */
		/* both strands: values done (the fold begins; ev[3] is then "folded"), reverse range aligned, forward rows moved, strand take
		 * begins, strands taken */
		hipEvent_t evs[5] = {};
		~Sync()
		{
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
			for (hipEvent_t e : ev)
				if (e)
					(void)hipEventDestroy(e);
			for (hipEvent_t e : evs)
				if (e)
					(void)hipEventDestroy(e);
		}
	} sy;
	SA_HIP_CHECK(hipStreamCreateWithFlags(&sy.s, hipStreamNonBlocking), return nullptr);
	for (hipEvent_t &e : sy.ev)
		SA_HIP_CHECK(hipEventCreate(&e), return nullptr);
	if (strands) {
		for (hipEvent_t &e : sy.evs)
			SA_HIP_CHECK(hipEventCreate(&e), return nullptr);
	}
	struct Res {
		sa_hitlist *h = nullptr;
		~Res() { delete h; }
	} res;
	res.h = new sa_hitlist;
	sa_hitlist *h = res.h;
	h->queries = (int32_t)m;
	h->offsets = static_cast<int64_t *>(malloc(sizeof(int64_t) * ((size_t)m + 1)));
	if (!h->offsets || !grow(&h->index, 0) || !grow(&h->value, 0) || (quantity && !grow(&h->score, 0))) {
		sa_set_error("%s: out of host memory for the offsets of %lld queries", who, (long long)m);
		return nullptr;
	}
	h->offsets[0] = 0;
	const size_t arrays = quantity ? 3 : 2; /* device: index, value and, under a quantity, score */
	std::vector<int32_t> h_den(norm && norm->denominators ? dens : 0);
	std::vector<int64_t> h_off((size_t)nqb + 1);
	double t_align = 0.0, t_gather = 0.0, t_quantity = 0.0, t_above = 0.0, t_strands = 0.0;
	int32_t batches = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = (int32_t)std::min<int64_t>(nqb, m - q0);
		int32_t *const dr = static_cast<int32_t *>(d_rect.p), *const dv = quantity ? static_cast<int32_t *>(d_vrect.p) : dr;
		int64_t *const dsc = static_cast<int64_t *>(d_scratch.p), *const doff = static_cast<int64_t *>(d_offsets.p);
		int32_t *const drr = static_cast<int32_t *>(d_rrev.p), *const dvr = quantity ? static_cast<int32_t *>(d_vrev.p) : drr;
		uint64_t *const dbits = static_cast<uint64_t *>(d_bits.p);
		SA_HIP_CHECK(hipEventRecord(sy.ev[0], sy.s), return nullptr);
		if (aligned) {
			if (sa_search_range_launch(ctx, (int32_t)q0, nq, dr, d_range.p, sy.s, sy.ev[1]) != 0)
				return nullptr;
			if (strands) { /* the rows M + q0 .. through the same buffer of the range */
				SA_HIP_CHECK(hipEventRecord(sy.evs[2], sy.s), return nullptr);
				if (sa_search_range_launch(ctx, (int32_t)(m + q0), nq, drr, d_range.p, sy.s, sy.evs[1]) != 0)
					return nullptr;
			}
			SA_HIP_CHECK(hipEventRecord(sy.ev[2], sy.s), return nullptr);
			if (norm) {
				if (q0 == 0) { /* once per call */
					SA_HIP_CHECK(sa_denominators_launch(ctx, norm->source, static_cast<int32_t *>(d_den.p), sy.s), return nullptr);
				}
				if (sa_normalize_rect_launch(dr, (int32_t)n, (int32_t)q0, nq, static_cast<const int32_t *>(d_den.p), norm->rule, dv, sy.s) != 0)
					return nullptr;
				if (strands && sa_normalize_rect_launch(drr, (int32_t)n, (int32_t)(m + q0), nq, static_cast<const int32_t *>(d_den.p), norm->rule,
									 dvr, sy.s) != 0)
					return nullptr;
			}
		} else {
			const struct sa_identity_out out = { dr, nullptr, nullptr, dv, *pid_denom }, rev = { drr, nullptr, nullptr, dvr, *pid_denom };
			SA_HIP_CHECK(hipEventRecord(sy.ev[1], sy.s), return nullptr);
			if (strands) {
				SA_HIP_CHECK(hipEventRecord(sy.evs[2], sy.s), return nullptr);
				SA_HIP_CHECK(hipEventRecord(sy.evs[1], sy.s), return nullptr);
			}
			SA_HIP_CHECK(hipEventRecord(sy.ev[2], sy.s), return nullptr);
			if (!sa_identity_rect(who, ctx, (int32_t)q0, nq, &out, sy.s) || (strands && !sa_identity_rect(who, ctx, (int32_t)(m + q0), nq, &rev, sy.s)))
				return nullptr;
		}
		if (strands) { /* in place: the folded values replace the forward values, the folded raw scores the forward raw scores */
			SA_HIP_CHECK(hipEventRecord(sy.evs[0], sy.s), return nullptr);
			if (sa_strand_fold_launch(dv, dvr, quantity ? dr : nullptr, quantity ? drr : nullptr, (int32_t)n, nq, dv, quantity ? dr : nullptr, dbits,
						  sy.s) != 0)
				return nullptr;
		}
		SA_HIP_CHECK(hipEventRecord(sy.ev[3], sy.s), return nullptr);
		if (offsets_launch(dv, (int32_t)n, nq, min_value, doff, dsc, sy.s) != 0)
			return nullptr;
		SA_HIP_CHECK(hipEventRecord(sy.ev[4], sy.s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(h_off.data(), doff, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToHost, sy.s), return nullptr);
		if (q0 == 0 && !h_den.empty()) {
			SA_HIP_CHECK(hipMemcpyAsync(h_den.data(), d_den.p, sizeof(int32_t) * h_den.size(), hipMemcpyDeviceToHost, sy.s), return nullptr);
		}
		SA_HIP_CHECK(hipStreamSynchronize(sy.s), return nullptr); /* E of the batch */
		const int64_t e = h_off[(size_t)nq], at = h->count;
		const size_t elems = (size_t)e, total = (size_t)(at + e);
		const double gib = (double)elems * 4.0 * (double)arrays / (double)(1 << 30);
		float ms_fill = 0.f, ms_take = 0.f;
		if (elems) {
			const size_t out_bytes = sizeof(int32_t) * arrays * elems + (strands ? elems : 0); /* (the strands: one byte per hit, last) */
			if (d_out.bytes < out_bytes) { /* exact; the largest so far is kept */
				(void)hipFree(d_out.p);
				d_out.p = nullptr;
				d_out.bytes = 0;
				if (hipMalloc(&d_out.p, out_bytes) != hipSuccess) {
					(void)hipGetLastError();
					d_out.p = nullptr;
					sa_set_error("%s: the %lld hits of queries [%lld,+%d) (%.2f GiB) do not fit the device's memory", who, (long long)e,
						     (long long)q0, nq, gib);
					return nullptr;
				}
				d_out.bytes = out_bytes;
			}
			if (!grow(&h->index, total) || !grow(&h->value, total) || (quantity && !grow(&h->score, total)) || (strands && !grow8(&h->strand, total))) {
				sa_set_error("%s: the %lld hits of queries [%lld,+%d) (%.2f GiB, %lld hits before them) do not fit the host's memory", who,
					     (long long)e, (long long)q0, nq, gib, (long long)at);
				return nullptr;
			}
			int32_t *const di = static_cast<int32_t *>(d_out.p), *const dval = di + elems, *const dscore = quantity ? di + 2 * elems : nullptr;
			SA_HIP_CHECK(hipEventRecord(sy.ev[5], sy.s), return nullptr);
			if (fill_launch(dv, dr, (int32_t)n, nq, min_value, doff, dsc, di, dval, dscore, sy.s) != 0)
				return nullptr;
			SA_HIP_CHECK(hipEventRecord(sy.ev[6], sy.s), return nullptr);
			if (strands) {
				uint8_t *const dstrand = reinterpret_cast<uint8_t *>(di + arrays * elems);
				SA_HIP_CHECK(hipEventRecord(sy.evs[3], sy.s), return nullptr);
				if (sa_hits_above_strand_launch(dbits, (int32_t)n, nq, doff, di, dstrand, sy.s) != 0)
					return nullptr;
				SA_HIP_CHECK(hipEventRecord(sy.evs[4], sy.s), return nullptr);
				SA_HIP_CHECK(hipMemcpyAsync(h->strand + at, dstrand, elems, hipMemcpyDeviceToHost, sy.s), return nullptr);
			}
			SA_HIP_CHECK(hipMemcpyAsync(h->index + at, di, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return nullptr);
			SA_HIP_CHECK(hipMemcpyAsync(h->value + at, dval, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return nullptr);
			if (quantity) {
				SA_HIP_CHECK(hipMemcpyAsync(h->score + at, dscore, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return nullptr);
			}
			SA_HIP_CHECK(hipStreamSynchronize(sy.s), return nullptr); /* (the next batch reuses the buffers) */
			SA_HIP_CHECK(hipEventElapsedTime(&ms_fill, sy.ev[5], sy.ev[6]), return nullptr);
			if (strands) {
				SA_HIP_CHECK(hipEventElapsedTime(&ms_take, sy.evs[3], sy.evs[4]), return nullptr);
			}
		}
		for (int32_t r = 0; r < nq; r++)
			h->offsets[q0 + r + 1] = at + h_off[(size_t)r + 1];
		h->count = at + e;
		float ms[4] = {};
		for (int t = 0; t < 4; t++)
			SA_HIP_CHECK(hipEventElapsedTime(&ms[t], sy.ev[t], sy.ev[t + 1]), return nullptr);
		if (strands) { /* the reverse half of alignment and gather; the fold is no part of the quantity */
			float a = 0.f, g0 = 0.f, g1 = 0.f, q = 0.f, f = 0.f;
			SA_HIP_CHECK(hipEventElapsedTime(&g0, sy.ev[1], sy.evs[2]), return nullptr);
			SA_HIP_CHECK(hipEventElapsedTime(&a, sy.evs[2], sy.evs[1]), return nullptr);
			SA_HIP_CHECK(hipEventElapsedTime(&g1, sy.evs[1], sy.ev[2]), return nullptr);
			SA_HIP_CHECK(hipEventElapsedTime(&q, sy.ev[2], sy.evs[0]), return nullptr);
			SA_HIP_CHECK(hipEventElapsedTime(&f, sy.evs[0], sy.ev[3]), return nullptr);
			ms[0] += a;
			ms[1] = g0 + g1;
			ms[2] = q;
			t_strands += ((double)f + (double)ms_take) * 1e-3;
		}
		t_align += (double)ms[0] * 1e-3;
		t_gather += (double)ms[1] * 1e-3;
		t_quantity += (double)ms[2] * 1e-3;
		t_above += ((double)ms[3] + (double)ms_fill) * 1e-3;
		batches++;
	}
	if (strands) {
		if (!h->strand && !grow8(&h->strand, 0)) { /* (never a null pointer for a valid result) */
			sa_set_error("%s: out of host memory", who);
			return nullptr;
		}
		sa_strands_last_set(t_strands);
	}
	if (!quantity)
		h->score = h->value; /* raw scores: value == score, one array */
	if (!h_den.empty())
		std::copy(h_den.begin(), h_den.end(), norm->denominators);
	g_last_above_seconds.store(t_above);
	sa_search_quantity_last_set(quantity ? t_quantity : 0.0);
	/* (under percent identity the sweep is the alignment as well: it is what delivers the scores) */
	sa_search_last_set(aligned ? t_align : t_quantity, t_gather, t_above, batches);
	res.h = nullptr;
	return h;
}

} // namespace

extern "C" size_t sa_hits_above_scratch_bytes(int32_t n_db, int32_t nq)
{
	return sa_guard("sa_hits_above_scratch_bytes", (size_t)0, [&]() -> size_t {
		if (n_db < 1 || nq < 1)
			return 0;
		return sizeof(int64_t) * (size_t)sa_above_scratch_elems(n_db, nq);
	});
}

extern "C" int sa_ctx_hits_above_offsets(sa_ctx *ctx, const int32_t *d_vrect, int32_t nq, int32_t min_value, int64_t *d_offsets, void *d_scratch,
					 void *stream)
{
	return sa_guard("sa_ctx_hits_above_offsets", 1, [&] {
		const char *who = "sa_ctx_hits_above_offsets";
		if (!sa_search_ctx_check(who, ctx))
			return 1;
		if (!d_vrect || !d_offsets || !d_scratch) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if (!above_check(who, ctx, nq, d_scratch))
			return 1;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return offsets_launch(d_vrect, ctx->search_db, nq, min_value, d_offsets, static_cast<int64_t *>(d_scratch), (hipStream_t)stream);
	});
}

extern "C" int sa_ctx_hits_above_fill(sa_ctx *ctx, const int32_t *d_vrect, const int32_t *d_rect, int32_t nq, int32_t min_value,
				      const int64_t *d_offsets, const void *d_scratch, int32_t *d_index, int32_t *d_value, int32_t *d_score, void *stream)
{
	return sa_guard("sa_ctx_hits_above_fill", 1, [&] {
		const char *who = "sa_ctx_hits_above_fill";
		if (!sa_search_ctx_check(who, ctx))
			return 1;
		if (!d_vrect || !d_offsets || !d_scratch || !d_index || (d_score && !d_rect)) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if (!above_check(who, ctx, nq, d_scratch))
			return 1;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return fill_launch(d_vrect, d_rect, ctx->search_db, nq, min_value, d_offsets, static_cast<const int64_t *>(d_scratch), d_index, d_value,
				   d_score, (hipStream_t)stream);
	});
}

extern "C" sa_hitlist *sa_hip_search_above(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t min_value,
					   const struct sa_norm *norm, const int32_t *pid_denom)
{
	return sa_guard("sa_hip_search_above", (sa_hitlist *)nullptr, [&] { return above_impl(db, queries, sc, min_value, norm, pid_denom); });
}

extern "C" const int64_t *sa_hitlist_offsets(const sa_hitlist *h, int32_t *queries)
{
	return sa_guard("sa_hitlist_offsets", (const int64_t *)nullptr, [&] {
		if (queries)
			*queries = h ? h->queries : 0;
		return h ? (const int64_t *)h->offsets : nullptr;
	});
}

extern "C" const int32_t *sa_hitlist_index(const sa_hitlist *h, int64_t *count)
{
	return sa_guard("sa_hitlist_index", (const int32_t *)nullptr, [&] {
		if (count)
			*count = h ? h->count : 0;
		return h ? (const int32_t *)h->index : nullptr;
	});
}

extern "C" const int32_t *sa_hitlist_value(const sa_hitlist *h)
{
	return sa_guard("sa_hitlist_value", (const int32_t *)nullptr, [&] { return h ? (const int32_t *)h->value : nullptr; });
}

extern "C" const int32_t *sa_hitlist_score(const sa_hitlist *h)
{
	return sa_guard("sa_hitlist_score", (const int32_t *)nullptr, [&] { return h ? (const int32_t *)h->score : nullptr; });
}

extern "C" sa_hitlist *sa_hip_search_above_strands(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp,
						   int32_t min_value, const struct sa_norm *norm, const int32_t *pid_denom)
{
	return sa_guard("sa_hip_search_above_strands", (sa_hitlist *)nullptr,
			[&] { return above_impl(db, queries, sc, min_value, norm, pid_denom, true, comp); });
}

extern "C" const uint8_t *sa_hitlist_strand(const sa_hitlist *h)
{
	return sa_guard("sa_hitlist_strand", (const uint8_t *)nullptr, [&] { return h ? (const uint8_t *)h->strand : nullptr; });
}

extern "C" void sa_hitlist_destroy(sa_hitlist *h)
{
	sa_guard_void("sa_hitlist_destroy", [&] { delete h; });
}

extern "C" double sa_hip_last_search_above_seconds(void)
{
	return sa_guard("sa_hip_last_search_above_seconds", 0.0, [&] { return g_last_above_seconds.load(); });
}
