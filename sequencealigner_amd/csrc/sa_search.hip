/*
 * sa_search.hip -- queries against a database: the M x N rectangle of a search context and the k best database sequences
 * of every query, selected where the scores are (sa_ctx_search_range, sa_ctx_hits, sa_hip_search).  No reference
 * counterpart: the reference scores one store against itself.
 *
 * A search context (sa_context.hip: sa_ctx_create_search) holds db followed by queries as ONE store whose plans are bounded
 * to the rows below N = the database size (sa_plan.h: row_end).  The score of query q against database sequence d is pair
 * (d, N + q) of that store, so queries [q0, q0 + nq) are the packed range [tri(N + q0), tri(N + q0 + nq)) with every column
 * cut to its first N rows: the systolic kernels run it as they run any range, nq * N pairs and no query-query pair, and store
 * column N + q at its packed place -- row q at pitch N + q.  sa_k_rect_rows then moves the rows to the dense pitch N.  (The
 * kernels' store epilogues place scores by packed index; a dense store straight from them is left out.)
 *
 * Hits.  A row of the rectangle is scanned by waves, 64 candidates per step, the k-entry list one entry per lane exactly as
 * in sa_neighbors.hip: compare with the k-th entry by readlane, ballot, population count for the position, a one-lane DPP
 * shift.  What differs is who owns a row.  sa_k_neighbors gives whole rows to a workgroup; with three queries and a million
 * database sequences that is three waves.  Here every row is cut into S segments (sa_search_core.h: sa_hits_segments) and
 * sa_k_hits_part runs one wave per (row, segment), which leaves k keys per segment in scratch; sa_k_hits_merge, one wave per
 * row, inserts those S * k keys.  The key is unique per candidate, so the cut cannot change a result.  With S = 1 phase 1
 * writes the result itself and there is no phase 2.
 */
#include <cstdint>
#include <mutex>

#include "sa_search_core.h"
#include "sa_search_run.h"

namespace {

constexpr int SR_THREADS = 256; /* four waves */

/* ---- rectangle: rows of the bounded range to their dense places ---------------------------------------------------- */
/* One workgroup moves pieces of SR_THREADS * 4 consecutive elements of one row: loads and stores run along d.  Every
 * offset is 64-bit (a batch's range and rectangle may pass 2^31 elements). */
__global__ __launch_bounds__(SR_THREADS) void sa_k_rect_rows(const int32_t *__restrict__ range, int32_t n_db, int32_t q0, int32_t nq,
							     int32_t *__restrict__ rect)
{
	constexpr int PIECE = SR_THREADS * 4;
	const int64_t per_row = ((int64_t)n_db + PIECE - 1) / PIECE, pieces = per_row * nq;
	for (int64_t p = blockIdx.x; p < pieces; p += gridDim.x) {
		const int64_t r = p / per_row, d0 = (p - r * per_row) * PIECE;
		const int32_t *src = range + sa_search_row_at(n_db, q0, (int64_t)q0 + r);
		int32_t *dst = rect + r * (int64_t)n_db;
		int32_t v[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t d = d0 + u * SR_THREADS + threadIdx.x;
			v[u] = d < n_db ? src[d] : 0;
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t d = d0 + u * SR_THREADS + threadIdx.x;
			if (d < n_db)
				dst[d] = v[u];
		}
	}
}

/* ---- hits ------------------------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint64_t sr_readlane(uint64_t v, int lane) /* lane: wave-uniform */
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
	return ((uint64_t)hi << 32) | lo;
}

/* lane l receives lane l - 1's value (wave_shr:1, all 64 lanes); lane 0 keeps its own */
__device__ __forceinline__ uint64_t sr_shift_down(uint64_t v)
{
	const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
	const uint32_t slo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
	const uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
	return ((uint64_t)shi << 32) | slo;
}

/* one step: the wave's 64 candidate keys x (SA_NB_EMPTY: none) against the list `mine` (one entry per lane, descending) */
__device__ __forceinline__ void sr_step(uint64_t &mine, uint64_t &kth, const uint64_t x, const int32_t k, const int lane)
{
	uint64_t pass = __ballot(x > kth);
	while (pass) {
		const int from = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(pass));
		pass &= pass - 1;
		const uint64_t cand = sr_readlane(x, from);
		if (cand > kth) { /* (the k-th entry has moved since the ballot) */
			const int pos = __popcll(__ballot(mine > cand));
			const uint64_t above = sr_shift_down(mine);
			mine = lane < pos ? mine : lane == pos ? cand : above;
			kth = sr_readlane(mine, k - 1);
		}
	}
}

/* Phase 1: wave w of the grid scans segment w % S of row w / S.  S > 1: its k keys go to part[(row * S + seg) * k ...];
 * S = 1: index / score of the row are written here. */
__global__ __launch_bounds__(SR_THREADS) void sa_k_hits_part(const int32_t *__restrict__ rect, int32_t n_db, int32_t nq, int32_t k, int32_t S,
							     uint64_t *__restrict__ part, int32_t *__restrict__ index, int32_t *__restrict__ score)
{
	const int lane = threadIdx.x & 63;
	const int64_t w = (int64_t)blockIdx.x * (SR_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (w >= (int64_t)nq * S) /* (wave-uniform) */
		return;
	const int64_t r = w / S;
	const int32_t seg = (int32_t)(w - r * S);
	const int32_t c0 = sa_hits_seg_begin(n_db, S, seg), c1 = sa_hits_seg_begin(n_db, S, seg + 1);
	const int32_t *row = rect + r * (int64_t)n_db;
	uint64_t mine = SA_NB_EMPTY, kth = SA_NB_EMPTY;
	int64_t c = (int64_t)c0 + lane; /* (64-bit: c1 + 63 may pass INT32_MAX) */
	int32_t v = c < c1 ? row[c] : 0;
	for (int64_t b = c0; b < c1; b += 64) {
		const int64_t cn = c + 64;
		const int32_t vn = cn < c1 ? row[cn] : 0; /* in flight while this step is scanned */
		const uint64_t x = c < c1 ? sa_nb_key(v, (int32_t)c) : SA_NB_EMPTY;
		sr_step(mine, kth, x, k, lane);
		c = cn;
		v = vn;
	}
	if (lane < k) {
		if (S > 1) {
			part[w * k + lane] = mine;
		} else {
			index[r * k + lane] = sa_nb_key_index(mine);
			score[r * k + lane] = sa_nb_key_score(mine);
		}
	}
}

/* Phase 2: one wave per row inserts the S * k keys of its partial lists */
__global__ __launch_bounds__(SR_THREADS) void sa_k_hits_merge(const uint64_t *__restrict__ part, int32_t nq, int32_t k, int32_t S,
							      int32_t *__restrict__ index, int32_t *__restrict__ score)
{
	const int lane = threadIdx.x & 63;
	const int64_t r = (int64_t)blockIdx.x * (SR_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (r >= nq) /* (wave-uniform) */
		return;
	const int32_t n = S * k; /* (<= SA_HITS_SEG_MAX * 64) */
	const uint64_t *keys = part + r * (int64_t)n;
	uint64_t mine = SA_NB_EMPTY, kth = SA_NB_EMPTY;
	uint64_t x = lane < n ? keys[lane] : SA_NB_EMPTY;
	for (int32_t b = 0; b < n; b += 64) {
		const int32_t tn = b + 64 + lane;
		const uint64_t xn = tn < n ? keys[tn] : SA_NB_EMPTY;
		sr_step(mine, kth, x, k, lane);
		x = xn;
	}
	if (lane < k) {
		index[r * k + lane] = sa_nb_key_index(mine);
		score[r * k + lane] = sa_nb_key_score(mine);
	}
}

std::mutex g_last_mutex;
struct Last {
	double align = 0, gather = 0, hits = 0;
	int32_t batches = 0;
} g_last;

} // namespace

bool sa_hits_check(const char *who, int64_t n_db, int64_t nq, int32_t k)
{
	if (n_db < 1 || nq < 1 || n_db > INT32_MAX || nq > INT32_MAX) {
		sa_set_error("%s: %lld queries against %lld database sequences: both must be in [1, 2^31)", who, (long long)nq, (long long)n_db);
		return false;
	}
	if (k < 1 || k > SA_HIP_NEIGHBORS_MAX || (int64_t)k > n_db) {
		sa_set_error("%s: k = %d hits among %lld database sequences: k must be in [1, min(N, %d)]", who, k, (long long)n_db, SA_HIP_NEIGHBORS_MAX);
		return false;
	}
	return true;
}

bool sa_search_ctx_check(const char *who, const sa_ctx *ctx)
{
	if (!ctx) {
		sa_set_error("%s: null context", who);
		return false;
	}
	if (!ctx->search_db) {
		sa_set_error("%s: not a search context (sa_ctx_create_search)", who);
		return false;
	}
	return true;
}

bool sa_search_queries_check(const char *who, const sa_ctx *ctx, int32_t q0, int32_t nq)
{
	if (q0 < 0 || nq < 1 || q0 > ctx->search_queries - nq) {
		sa_set_error("%s: queries [%d,+%d) of %d", who, q0, nq, ctx->search_queries);
		return false;
	}
	return true;
}

/* the range into d_scratch, the rows into d_rect; `mid`, when not null, is recorded between the two */
int sa_search_range_launch(sa_ctx *ctx, int32_t q0, int32_t nq, int32_t *d_rect, void *d_scratch, hipStream_t s, hipEvent_t mid)
{
	const char *who = "sa_ctx_search_range";
	if (!sa_search_ctx_check(who, ctx) || !sa_search_queries_check(who, ctx, q0, nq))
		return 1;
	if (!d_rect || !d_scratch) {
		sa_set_error("%s: null buffer", who);
		return 1;
	}
	const int64_t n = ctx->search_db;
	const int64_t start = sa_search_tri(n + q0), count = sa_search_range_elems(n, q0, nq);
	if (sa_align_range_impl(ctx, start, count, static_cast<int32_t *>(d_scratch), s, false) != 0)
		return 1;
	if (mid) {
		SA_HIP_CHECK(hipEventRecord(mid, s), return 1);
	}
	constexpr int64_t PIECE = SR_THREADS * 4;
	const int64_t pieces = (n + PIECE - 1) / PIECE * nq;
	const unsigned grid = (unsigned)std::min<int64_t>(pieces, (int64_t)1 << 20);
	hipLaunchKernelGGL(sa_k_rect_rows, dim3(grid), dim3(SR_THREADS), 0, s, static_cast<const int32_t *>(d_scratch), (int32_t)n, q0, nq, d_rect);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

int sa_hits_launch(const int32_t *d_rect, int32_t n_db, int32_t nq, int32_t k, int32_t *d_index, int32_t *d_score, void *d_scratch, hipStream_t s)
{
	const int32_t S = sa_hits_segments(n_db, nq, k);
	constexpr int WPB = SR_THREADS / 64;
	const int64_t waves = (int64_t)nq * S;
	hipLaunchKernelGGL(sa_k_hits_part, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(SR_THREADS), 0, s, d_rect, n_db, nq, k, S,
			   static_cast<uint64_t *>(d_scratch), d_index, d_score);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	if (S > 1) {
		hipLaunchKernelGGL(sa_k_hits_merge, dim3((unsigned)(((int64_t)nq + WPB - 1) / WPB)), dim3(SR_THREADS), 0, s,
				   static_cast<const uint64_t *>(d_scratch), nq, k, S, d_index, d_score);
		SA_HIP_CHECK(hipGetLastError(), return 1);
	}
	return 0;
}

void sa_search_last_set(double align, double gather, double hits, int32_t batches)
{
	std::lock_guard<std::mutex> g(g_last_mutex);
	g_last.align = align;
	g_last.gather = gather;
	g_last.hits = hits;
	g_last.batches = batches;
}

namespace {

bool search_impl(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score, int32_t *rect)
{
	const char *who = "sa_hip_search";
	if (!sc) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	const bool want_hits = index || score;
	if (want_hits && (!index || !score)) {
		sa_set_error("%s: index and score go together", who);
		return false;
	}
	if (!want_hits && !rect) {
		sa_set_error("%s: nothing asked for (index / score and rect are all null)", who);
		return false;
	}
	if (!sa_run_stores_not_empty(who, db, queries) || !sa_run_stores_not_null(who, db, queries))
		return false;
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	if (!sa_run_device_check())
		return false;
	SearchRun run(who);
	if (!run.adopt(sa_ctx_create_search(0, db, queries, sc), db, queries))
		return false;
	RectStage stage(run, nullptr, nullptr, false);
	if (!stage.begin(sa_batch_tail_topk(want_hits, false, false, k)))
		return false;
	const int32_t n = (int32_t)run.n;
	const size_t cap = (size_t)run.nqb * (size_t)k;
	int32_t *di = nullptr;
	void *d_part = nullptr;
	if (want_hits && (!run.alloc(di, 2 * sizeof(int32_t) * cap, "the hits of a query batch") ||
			  !run.alloc(d_part, run.largest([&](int32_t, int32_t nq) { return sa_hits_scratch_bytes(n, nq, k); }), "the partial hit lists")))
		return false;
	int32_t *const ds = di ? di + cap : nullptr, *const dr = stage.raw();
	if (!run.start())
		return false;
	const bool ok = run.each_batch([&](int64_t q0, int32_t nq) {
		hipStream_t s = run.sy.s;
		const size_t hits = sizeof(int32_t) * (size_t)nq * (size_t)k;
		if (!stage.launch(q0, nq))
			return false;
		if (want_hits && (!run.stamp(SA_PH_SELECT) || sa_hits_launch(dr, n, nq, k, di, ds, d_part, s) != 0))
			return false;
		if (!run.stamp(SA_PH_END))
			return false;
		if (rect) {
			SA_HIP_CHECK(hipMemcpyAsync(rect + q0 * n, dr, sizeof(int32_t) * (size_t)nq * (size_t)n, hipMemcpyDeviceToHost, s), return false);
		}
		if (want_hits) {
			SA_HIP_CHECK(hipMemcpyAsync(index + q0 * k, di, hits, hipMemcpyDeviceToHost, s), return false);
			SA_HIP_CHECK(hipMemcpyAsync(score + q0 * k, ds, hits, hipMemcpyDeviceToHost, s), return false);
		}
		return true;
	});
	if (!ok)
		return false;
	const PhaseClock &t = run.sy.clock;
	sa_search_last_set(t[SA_PH_ALIGN], t[SA_PH_GATHER], t[SA_PH_SELECT], run.batches);
	return true;
}

} // namespace

extern "C" size_t sa_search_scratch_bytes(const sa_ctx *ctx, int32_t q0, int32_t nq)
{
	return sa_guard("sa_search_scratch_bytes", (size_t)0, [&]() -> size_t {
		if (!ctx || !ctx->search_db || q0 < 0 || nq < 1 || q0 > ctx->search_queries - nq)
			return 0;
		return sizeof(int32_t) * (size_t)sa_search_range_elems(ctx->search_db, q0, nq);
	});
}

extern "C" int sa_ctx_search_range(sa_ctx *ctx, int32_t q0, int32_t nq, int32_t *d_rect, void *d_scratch, void *stream)
{
	return sa_guard("sa_ctx_search_range", 1, [&] { return sa_search_range_launch(ctx, q0, nq, d_rect, d_scratch, (hipStream_t)stream, nullptr); });
}

extern "C" size_t sa_hits_scratch_bytes(int32_t n_db, int32_t nq, int32_t k)
{
	return sa_guard("sa_hits_scratch_bytes", (size_t)0, [&]() -> size_t {
		if (n_db < 1 || nq < 1 || k < 1 || k > SA_HIP_NEIGHBORS_MAX || k > n_db)
			return 0;
		const int32_t S = sa_hits_segments(n_db, nq, k);
		return S > 1 ? sizeof(uint64_t) * (size_t)nq * (size_t)S * (size_t)k : 0;
	});
}

extern "C" int sa_ctx_hits(sa_ctx *ctx, const int32_t *d_rect, int32_t nq, int32_t k, int32_t *d_index, int32_t *d_score, void *d_scratch,
			   void *stream)
{
	return sa_guard("sa_ctx_hits", 1, [&] {
		const char *who = "sa_ctx_hits";
		if (!sa_search_ctx_check(who, ctx))
			return 1;
		if (!d_rect || !d_index || !d_score) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if (!sa_hits_check(who, ctx->search_db, nq, k))
			return 1;
		if (nq > ctx->search_queries) {
			sa_set_error("%s: %d rows, the context has %d queries", who, nq, ctx->search_queries);
			return 1;
		}
		if (!d_scratch && sa_hits_scratch_bytes(ctx->search_db, nq, k) > 0) {
			sa_set_error("%s: null scratch (sa_hits_scratch_bytes: %zu bytes)", who, sa_hits_scratch_bytes(ctx->search_db, nq, k));
			return 1;
		}
		if (reinterpret_cast<uintptr_t>(d_scratch) % alignof(uint64_t)) { /* (the partial lists are 64-bit keys) */
			sa_set_error("%s: scratch not 8-byte aligned", who);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return sa_hits_launch(d_rect, ctx->search_db, nq, k, d_index, d_score, d_scratch, (hipStream_t)stream);
	});
}

extern "C" bool sa_hip_search(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index,
			      int32_t *score, int32_t *rect)
{
	return sa_guard("sa_hip_search", false, [&] { return search_impl(db, queries, sc, k, index, score, rect); });
}

extern "C" double sa_hip_last_search_seconds(void)
{
	return sa_guard("sa_hip_last_search_seconds", 0.0, [&] {
		std::lock_guard<std::mutex> g(g_last_mutex);
		return g_last.align + g_last.gather + g_last.hits;
	});
}

extern "C" void sa_hip_last_search_breakdown(double *align, double *gather, double *hits, int32_t *batches)
{
	sa_guard_void("sa_hip_last_search_breakdown", [&] {
		std::lock_guard<std::mutex> g(g_last_mutex);
		if (align)
			*align = g_last.align;
		if (gather)
			*gather = g_last.gather;
		if (hits)
			*hits = g_last.hits;
		if (batches)
			*batches = g_last.batches;
	});
}
