/*
 * sa_search_quantity.hip -- the hits of a search ranked by a value instead of the raw score: normalised scores or percent
 * identity of the M x N rectangle of a search context (sa_ctx_normalize_rect, sa_ctx_identity_rect, sa_ctx_hits_take,
 * sa_hip_search_norm, sa_hip_search_pid).  No reference counterpart.  The contract is in include/seqalign_hip.h, the index
 * arithmetic in sa_search_quantity_core.h, which the host compiles as well.
 *
 *   sa_k_normalize_rect<RULE>  the streaming sweep of sa_k_normalize at rectangle pitch: 4 bytes in, 4 bytes out per entry plus the
 *                              database denominators.  A workgroup takes pieces of SA_SQ_PIECE consecutive elements of one row,
 *                              as sa_k_rect_rows cuts them; the query's denominator is one uniform load per piece.  A row begins
 *                              at byte 4 r N, any alignment: the head / 16-byte vector / tail scheme of norm_column, one vector
 *                              per thread; the database denominators come as unaligned 4-vectors.  Every entry is read and
 *                              written by the same thread, once: in place is as good as disjoint.  The value is
 *                              sa_norm_value_t<RULE> of sa_normalize_core.h.
 *   sa_k_hits_take             out[r k + t] = rect[r N + index[r k + t]], one thread per hit: the raw scores of hits that were
 *                              selected on a value rectangle.
 * The identity sweep in rectangle form is sa_k_identity<METHOD, true> of sa_identity.hip: one body with the triangle form.
 * Neither kernel shares state between workgroups: the same input gives the same bytes.
 */
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

#include "sa_search_quantity_core.h"
#include "sa_search_run.h"

namespace {

constexpr int SQ_THREADS = SA_SQ_PIECE / 4;
static_assert(SQ_THREADS == 256, "a piece is one 16-byte vector per thread of a four-wave workgroup");

typedef int32_t i32x4u __attribute__((ext_vector_type(4), aligned(4))); /* den[d .. d + 4): wherever d falls */

/* (no __restrict__ on in / out: they may be the same buffer) */
template <int RULE>
__global__ __launch_bounds__(SQ_THREADS) void sa_k_normalize_rect(const int32_t *in, const int32_t *__restrict__ den, int32_t n_db, int32_t q0,
								   int32_t nq, int32_t *out)
{
	const int32_t tid = (int32_t)threadIdx.x;
	const int64_t pieces = sa_sq_pieces(n_db, nq);
	for (int64_t p = blockIdx.x; p < pieces; p += gridDim.x) { /* (uniform in the workgroup) */
		int64_t r, d0;
		int32_t len, head, vecs;
		sa_sq_piece(n_db, p, &r, &d0, &len);
		const int64_t at = sa_sq_at(n_db, r, d0);
		const int32_t *src = in + at;
		int32_t *dst = out + at;
		const int32_t *dd = den + d0;
		const int32_t dq = den[(int64_t)n_db + q0 + r];
		sa_sq_split((uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)dst, len, &head, &vecs);
		for (int32_t e = tid; e < head; e += SQ_THREADS)
			dst[e] = sa_norm_value_t<RULE>(src[e], dd[e], dq);
		if (tid < vecs) {
			const int32_t e = head + 4 * tid;
			const int4 s = *reinterpret_cast<const int4 *>(src + e);
			const i32x4u d = *reinterpret_cast<const i32x4u *>(dd + e);
			int4 v;
			v.x = sa_norm_value_t<RULE>(s.x, d.x, dq);
			v.y = sa_norm_value_t<RULE>(s.y, d.y, dq);
			v.z = sa_norm_value_t<RULE>(s.z, d.z, dq);
			v.w = sa_norm_value_t<RULE>(s.w, d.w, dq);
			*reinterpret_cast<int4 *>(dst + e) = v;
		}
		const int32_t e = head + 4 * vecs + tid;
		if (e < len)
			dst[e] = sa_norm_value_t<RULE>(src[e], dd[e], dq);
	}
}

__global__ __launch_bounds__(256) void sa_k_hits_take(const int32_t *__restrict__ rect, int32_t n_db, int32_t nq, int32_t k,
						       const int32_t *__restrict__ index, int32_t *__restrict__ out)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t < (int64_t)nq * k)
		out[t] = sa_sq_take_one(rect, n_db, k, index, t);
}

std::atomic<double> g_last_quantity_seconds{ 0.0 };

} // namespace

/* the sweep of sa_ctx_normalize_rect, its arguments checked by the caller */
int sa_normalize_rect_launch(const int32_t *d_rect, int32_t n_db, int32_t q0, int32_t nq, const int32_t *d_den, int32_t rule, int32_t *d_out,
			     hipStream_t s)
{
	const unsigned grid = (unsigned)std::min<int64_t>(sa_sq_pieces(n_db, nq), (int64_t)1 << 20);
	switch (rule) {
	case SA_NORM_MIN:
		hipLaunchKernelGGL(sa_k_normalize_rect<SA_NORM_RULE_MIN>, dim3(grid), dim3(SQ_THREADS), 0, s, d_rect, d_den, n_db, q0, nq, d_out);
		break;
	case SA_NORM_MAX:
		hipLaunchKernelGGL(sa_k_normalize_rect<SA_NORM_RULE_MAX>, dim3(grid), dim3(SQ_THREADS), 0, s, d_rect, d_den, n_db, q0, nq, d_out);
		break;
	default:
		hipLaunchKernelGGL(sa_k_normalize_rect<SA_NORM_RULE_MEAN>, dim3(grid), dim3(SQ_THREADS), 0, s, d_rect, d_den, n_db, q0, nq, d_out);
		break;
	}
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

/* the launch of sa_ctx_hits_take, its arguments checked by the caller */
int sa_hits_take_launch(const int32_t *d_rect, int32_t n_db, int32_t nq, int32_t k, const int32_t *d_index, int32_t *d_out, hipStream_t s)
{
	const int64_t hits = (int64_t)nq * k;
	hipLaunchKernelGGL(sa_k_hits_take, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, s, d_rect, n_db, nq, k, d_index, d_out);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

void sa_search_quantity_last_set(double seconds) { g_last_quantity_seconds.store(seconds); }

namespace {

/* what the two one-call forms ask for */
struct Want {
	int32_t *index, *value, *score, *rect, *vrect;
};

/* norm != NULL: normalised scores; otherwise percent identity under `denom` */
bool quantity_impl(const char *who, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, const Want &w,
		   const struct sa_norm *norm, int32_t denom)
{
	if (!sc) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	const bool want_hits = w.index || w.value || w.score;
	if (want_hits && !w.index) {
		sa_set_error("%s: value and score belong to the hits of index, which is null", who);
		return false;
	}
	if (!want_hits && !w.rect && !w.vrect) {
		sa_set_error("%s: nothing asked for (index, rect and vrect are all null)", who);
		return false;
	}
	if (!sa_run_stores_not_empty(who, db, queries) || !sa_run_stores_not_null(who, db, queries))
		return false;
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	if (norm ? !sa_norm_check(who, norm) : !sa_identity_denom_check(who, denom))
		return false;
	if (!sa_run_device_check())
		return false;
	SearchRun run(who);
	if (!run.adopt(sa_ctx_create_search(0, db, queries, sc), db, queries))
		return false;
	RectStage stage(run, norm, norm ? nullptr : &denom, false);
	if (!stage.begin(sa_batch_tail_topk(want_hits, true, false, k)))
		return false;
	const int32_t n = (int32_t)run.n;
	const size_t cap = (size_t)run.nqb * (size_t)k;
	int32_t *di = nullptr;
	void *d_part = nullptr;
	if (want_hits && (!run.alloc(di, 3 * sizeof(int32_t) * cap, "the hits of a query batch") ||
			  !run.alloc(d_part, run.largest([&](int32_t, int32_t nq) { return sa_hits_scratch_bytes(n, nq, k); }), "the partial hit lists")))
		return false;
	int32_t *const dval = di ? di + cap : nullptr, *const dsc = di ? di + 2 * cap : nullptr;
	int32_t *const dr = stage.raw(), *const dv = stage.value();
	if (!run.start())
		return false;
	const bool ok = run.each_batch([&](int64_t q0, int32_t nq) {
		hipStream_t s = run.sy.s;
		const size_t hits = sizeof(int32_t) * (size_t)nq * (size_t)k, elems = sizeof(int32_t) * (size_t)nq * (size_t)n;
		if (!stage.launch(q0, nq))
			return false;
		if (want_hits && (!run.stamp(SA_PH_SELECT) || sa_hits_launch(dv, n, nq, k, di, dval, d_part, s) != 0 ||
				  sa_hits_take_launch(dr, n, nq, k, di, dsc, s) != 0))
			return false;
		if (!run.stamp(SA_PH_END))
			return false;
		if (want_hits) {
			SA_HIP_CHECK(hipMemcpyAsync(w.index + q0 * k, di, hits, hipMemcpyDeviceToHost, s), return false);
			if (w.value) {
				SA_HIP_CHECK(hipMemcpyAsync(w.value + q0 * k, dval, hits, hipMemcpyDeviceToHost, s), return false);
			}
			if (w.score) {
				SA_HIP_CHECK(hipMemcpyAsync(w.score + q0 * k, dsc, hits, hipMemcpyDeviceToHost, s), return false);
			}
		}
		if (w.rect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.rect + q0 * n, dr, elems, hipMemcpyDeviceToHost, s), return false);
		}
		if (w.vrect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.vrect + q0 * n, dv, elems, hipMemcpyDeviceToHost, s), return false);
		}
		return stage.copy_denominators(q0);
	});
	if (!ok)
		return false;
	stage.publish_denominators();
	const PhaseClock &t = run.sy.clock;
	g_last_quantity_seconds.store(t[SA_PH_QUANTITY]);
	/* (under percent identity the sweep is the alignment as well: it is what delivers the scores) */
	sa_search_last_set(norm ? t[SA_PH_ALIGN] : t[SA_PH_QUANTITY], t[SA_PH_GATHER], t[SA_PH_SELECT], run.batches);
	return true;
}

/* norm == NULL: sa_hip_search, value a copy of score and vrect a copy of rect */
bool search_plain(const char *who, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, const Want &w)
{
	const bool want_hits = w.index || w.value || w.score;
	if (want_hits && !w.index) {
		sa_set_error("%s: value and score belong to the hits of index, which is null", who);
		return false;
	}
	if (!want_hits && !w.rect && !w.vrect) {
		sa_set_error("%s: nothing asked for (index, rect and vrect are all null)", who);
		return false;
	}
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	const size_t hits = want_hits && db.num > 0 && queries.num > 0 ? (size_t)queries.num * (size_t)k : 0;
	const size_t elems = db.num > 0 && queries.num > 0 ? (size_t)queries.num * (size_t)db.num : 0;
	std::vector<int32_t> tmp(want_hits && !w.score && !w.value ? hits : 0);
	int32_t *const score = !want_hits ? nullptr : w.score ? w.score : w.value ? w.value : tmp.data();
	int32_t *const rect = w.rect ? w.rect : w.vrect;
	if (!sa_hip_search(db, queries, sc, k, w.index, score, rect))
		return false;
	if (w.value && w.value != score)
		std::copy(score, score + hits, w.value);
	if (w.vrect && w.vrect != rect)
		std::copy(rect, rect + elems, w.vrect);
	g_last_quantity_seconds.store(0.0);
	return true;
}

} // namespace

extern "C" int sa_ctx_normalize_rect(sa_ctx *ctx, const int32_t *d_rect, int32_t nq, int32_t q0, const int32_t *d_den, int32_t rule,
				     int32_t *d_out, void *stream)
{
	return sa_guard("sa_ctx_normalize_rect", 1, [&] {
		const char *who = "sa_ctx_normalize_rect";
		if (!sa_search_ctx_check(who, ctx))
			return 1;
		if (!d_rect || !d_den || !d_out) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if (!sa_norm_rule_check(who, rule) || !sa_search_queries_check(who, ctx, q0, nq))
			return 1;
		if ((uintptr_t)d_rect % 4 || (uintptr_t)d_den % 4 || (uintptr_t)d_out % 4) {
			sa_set_error("%s: d_rect, d_den and d_out want 4-byte alignment", who);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return sa_normalize_rect_launch(d_rect, ctx->search_db, q0, nq, d_den, rule, d_out, (hipStream_t)stream);
	});
}

extern "C" int sa_ctx_identity_rect(sa_ctx *ctx, int32_t q0, int32_t nq, const struct sa_identity_out *d_out, void *stream)
{
	return sa_guard("sa_ctx_identity_rect", 1, [&] {
		const char *who = "sa_ctx_identity_rect";
		if (!sa_search_ctx_check(who, ctx) || !sa_search_queries_check(who, ctx, q0, nq))
			return 1;
		return sa_identity_rect(who, ctx, q0, nq, d_out, (hipStream_t)stream) ? 0 : 1;
	});
}

extern "C" int sa_ctx_hits_take(sa_ctx *ctx, const int32_t *d_rect, int32_t nq, int32_t k, const int32_t *d_index, int32_t *d_out, void *stream)
{
	return sa_guard("sa_ctx_hits_take", 1, [&] {
		const char *who = "sa_ctx_hits_take";
		if (!sa_search_ctx_check(who, ctx))
			return 1;
		if (!d_rect || !d_index || !d_out) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if (!sa_hits_check(who, ctx->search_db, nq, k))
			return 1;
		if (nq > ctx->search_queries) {
			sa_set_error("%s: %d rows, the context has %d queries", who, nq, ctx->search_queries);
			return 1;
		}
		if ((uintptr_t)d_rect % 4 || (uintptr_t)d_index % 4 || (uintptr_t)d_out % 4) {
			sa_set_error("%s: d_rect, d_index and d_out want 4-byte alignment", who);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return sa_hits_take_launch(d_rect, ctx->search_db, nq, k, d_index, d_out, (hipStream_t)stream);
	});
}

extern "C" bool sa_hip_search_norm(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index,
				   int32_t *value, int32_t *score, int32_t *rect, int32_t *vrect, const struct sa_norm *norm)
{
	return sa_guard("sa_hip_search_norm", false, [&] {
		const Want w = { index, value, score, rect, vrect };
		return norm ? quantity_impl("sa_hip_search_norm", db, queries, sc, k, w, norm, 0) : search_plain("sa_hip_search_norm", db, queries, sc, k, w);
	});
}

extern "C" bool sa_hip_search_pid(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t *index,
				  int32_t *value, int32_t *score, int32_t *rect, int32_t *vrect, int32_t denom)
{
	return sa_guard("sa_hip_search_pid", false, [&] {
		const Want w = { index, value, score, rect, vrect };
		return quantity_impl("sa_hip_search_pid", db, queries, sc, k, w, nullptr, denom);
	});
}

extern "C" double sa_hip_last_search_quantity_seconds(void)
{
	return sa_guard("sa_hip_last_search_quantity_seconds", 0.0, [&] { return g_last_quantity_seconds.load(); });
}
