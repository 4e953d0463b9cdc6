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

#include "sa_search_above_core.h"
#include "sa_search_run.h"

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

/* host arrays that grow with the batches */
template <class T> bool grow(T **p, size_t elems)
{
	void *q = realloc(*p, sizeof(T) * std::max<size_t>(elems, 1));
	if (!q)
		return false;
	*p = static_cast<T *>(q);
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
	if (!sa_run_stores_not_empty(who, db, queries) || !sa_run_stores_not_null(who, db, queries))
		return nullptr;
	if (norm && !sa_norm_check(who, norm))
		return nullptr;
	if (pid_denom && !sa_identity_denom_check(who, *pid_denom))
		return nullptr;
	uint8_t dna[SA_LUT_SIZE];
	sa_strands_complement_table(dna);
	const uint8_t *comp = comp_in ? comp_in : dna;
	if (strands && !sa_strands_inputs_check(who, db, queries, sc, comp))
		return nullptr;
	if (!sa_run_device_check())
		return nullptr;
	SearchRun run(who);
	if (!run.adopt(strands ? sa_ctx_create_search_strands(0, db, queries, sc, comp) : sa_ctx_create_search(0, db, queries, sc), db, queries))
		return nullptr;
	/* The tail of a batch is its segment counts: the entries of a batch are at most SA_HITS_WAVES + nq + 1, the rest is inside the
	 * quarter left free.  The hits themselves are sized once they are counted. */
	RectStage stage(run, norm, pid_denom, strands);
	if (!stage.begin(sa_batch_tail_above()))
		return nullptr;
	const int32_t n = (int32_t)run.n;
	const int64_t m = run.m;
	const bool quantity = stage.quantity;
	int64_t *dsc = nullptr, *doff = nullptr;
	if (!run.alloc(dsc, run.largest([&](int32_t, int32_t nq) { return sizeof(int64_t) * (size_t)sa_above_scratch_elems(n, nq); }), "the segment counts") ||
	    !run.alloc(doff, sizeof(int64_t) * ((size_t)run.nqb + 1), "the offsets of a query batch"))
		return nullptr;
	DevBuf &d_out = run.spare();
	if (!run.start())
		return nullptr;
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
	std::vector<int64_t> h_off((size_t)run.nqb + 1);
	int32_t *const dr = stage.raw(), *const dv = stage.value();
	const bool ok = run.each_batch([&](int64_t q0, int32_t nq) {
		hipStream_t s = run.sy.s;
		if (!stage.launch(q0, nq))
			return false;
		if (!run.stamp(SA_PH_SELECT) || offsets_launch(dv, n, nq, min_value, doff, dsc, s) != 0 || !run.stamp(SA_PH_END))
			return false;
		SA_HIP_CHECK(hipMemcpyAsync(h_off.data(), doff, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToHost, s), return false);
		if (!stage.copy_denominators(q0) || !run.sync()) /* E of the batch */
			return false;
		const int64_t e = h_off[(size_t)nq], at = h->count;
		const size_t elems = (size_t)e, total = (size_t)(at + e);
		const double gib = (double)elems * 4.0 * (double)arrays / (double)(1 << 30);
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
					return false;
				}
				d_out.bytes = out_bytes;
			}
			if (!grow(&h->index, total) || !grow(&h->value, total) || (quantity && !grow(&h->score, total)) || (strands && !grow(&h->strand, total))) {
				sa_set_error("%s: the %lld hits of queries [%lld,+%d) (%.2f GiB, %lld hits before them) do not fit the host's memory", who,
					     (long long)e, (long long)q0, nq, gib, (long long)at);
				return false;
			}
			int32_t *const di = static_cast<int32_t *>(d_out.p), *const dval = di + elems, *const dscore = quantity ? di + 2 * elems : nullptr;
			if (!run.stamp(SA_PH_FILL) || fill_launch(dv, dr, n, nq, min_value, doff, dsc, di, dval, dscore, s) != 0)
				return false;
			if (strands) {
				uint8_t *const dstrand = reinterpret_cast<uint8_t *>(di + arrays * elems);
				if (!run.stamp(SA_PH_STRAND_TAKE) || sa_hits_above_strand_launch(stage.bits(), n, nq, doff, di, dstrand, s) != 0 || !run.stamp(SA_PH_END))
					return false;
				SA_HIP_CHECK(hipMemcpyAsync(h->strand + at, dstrand, elems, hipMemcpyDeviceToHost, s), return false);
			} else if (!run.stamp(SA_PH_END)) {
				return false;
			}
			SA_HIP_CHECK(hipMemcpyAsync(h->index + at, di, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
			SA_HIP_CHECK(hipMemcpyAsync(h->value + at, dval, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
			if (quantity) {
				SA_HIP_CHECK(hipMemcpyAsync(h->score + at, dscore, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
			}
		}
		for (int32_t r = 0; r < nq; r++)
			h->offsets[q0 + r + 1] = at + h_off[(size_t)r + 1];
		h->count = at + e;
		return true;
	});
	if (!ok)
		return nullptr;
	const PhaseClock &t = run.sy.clock;
	const double t_above = t[SA_PH_SELECT] + t[SA_PH_FILL];
	if (strands) {
		if (!h->strand && !grow(&h->strand, 0)) { /* (never a null pointer for a valid result) */
			sa_set_error("%s: out of host memory", who);
			return nullptr;
		}
		sa_strands_last_set(t[SA_PH_FOLD] + t[SA_PH_STRAND_TAKE]); /* (the fold is no part of the quantity) */
	}
	if (!quantity)
		h->score = h->value; /* raw scores: value == score, one array */
	stage.publish_denominators();
	g_last_above_seconds.store(t_above);
	sa_search_quantity_last_set(t[SA_PH_QUANTITY]);
	/* (under percent identity the sweep is the alignment as well: it is what delivers the scores) */
	sa_search_last_set(stage.aligned ? t[SA_PH_ALIGN] : t[SA_PH_QUANTITY], t[SA_PH_GATHER], t_above, run.batches);
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
