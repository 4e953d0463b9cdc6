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

#include "sa_ctx.h"
#include "sa_search_quantity_core.h"

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

int normalize_rect_launch(const int32_t *d_rect, int32_t n_db, int32_t q0, int32_t nq, const int32_t *d_den, int32_t rule, int32_t *d_out,
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

int take_launch(const int32_t *d_rect, int32_t n_db, int32_t nq, int32_t k, const int32_t *d_index, int32_t *d_out, hipStream_t s)
{
	const int64_t hits = (int64_t)nq * k;
	hipLaunchKernelGGL(sa_k_hits_take, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, s, d_rect, n_db, nq, k, d_index, d_out);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

struct DevBuf {
	void *p = nullptr;
	~DevBuf() { (void)hipFree(p); }
	bool alloc(const char *who, size_t bytes, const char *what)
	{
		if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			sa_set_error("%s: %s (%.2f GiB) does not fit the device's memory", who, what, (double)bytes / (double)(1 << 30));
			return false;
		}
		return true;
	}
};

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
	if (db.num < 1 || queries.num < 1) {
		sa_set_error("%s: empty store (%d database sequences, %d queries; min: 1 each)", who, db.num, queries.num);
		return false;
	}
	if (!db.seqs || !db.meta || !queries.seqs || !queries.meta) {
		sa_set_error("%s: null sequence store", who);
		return false;
	}
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	if (norm ? !sa_norm_check(who, norm) : !sa_identity_denom_check(who, denom))
		return false;
	if (sa_hip_device_count() <= 0) {
		sa_set_error("No HIP devices available; libseqalign_hip has no CPU fallback");
		return false;
	}
	struct Ctx {
		sa_ctx *c = nullptr;
		~Ctx() { sa_ctx_destroy(c); }
	} cx;
	cx.c = sa_ctx_create_search(0, db, queries, sc);
	if (!cx.c)
		return false;
	sa_ctx *ctx = cx.c;
	const int64_t n = db.num, m = queries.num;
	/* Batch: as sa_hip_search sizes it, with the value rectangle counted.  Per query: the range row (the longest, N + M - 1
	 * elements; none under percent identity, which runs no packed alignment), a row of each rectangle, and with hits index,
	 * value, score and one partial list.  The identity sweep's payload scratch is the context's and is allocated before the free
	 * memory is read, as sa_hip_identity does it. */
	if (!norm && !sa_identity_payload_scratch(ctx))
		return false;
	size_t free_b = 0, total_b = 0;
	SA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b), return false);
	const int64_t per_query = (norm ? 4 * (n + m) : 0) + 8 * n + (want_hits ? 20 * (int64_t)k : 0);
	int64_t budget = (int64_t)(free_b - free_b / 4);
	if (ctx->env.search_batch_bytes > 0)
		budget = std::min<int64_t>(budget, ctx->env.search_batch_bytes);
	const int32_t nqb = (int32_t)std::max<int64_t>(1, std::min<int64_t>(m, budget / per_query));
	size_t scratch_bytes = 0, part_bytes = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = (int32_t)std::min<int64_t>(nqb, m - q0);
		if (norm)
			scratch_bytes = std::max(scratch_bytes, sa_search_scratch_bytes(ctx, (int32_t)q0, nq));
		if (want_hits)
			part_bytes = std::max(part_bytes, sa_hits_scratch_bytes((int32_t)n, nq, k));
	}
	DevBuf d_scratch, d_rect, d_vrect, d_den, d_hits, d_part;
	if ((norm && (!d_scratch.alloc(who, scratch_bytes, "the packed range of a query batch") ||
		      !d_den.alloc(who, sizeof(int32_t) * (size_t)(n + m), "the denominators"))) ||
	    !d_rect.alloc(who, sizeof(int32_t) * (size_t)nqb * (size_t)n, "the rectangle of a query batch") ||
	    !d_vrect.alloc(who, sizeof(int32_t) * (size_t)nqb * (size_t)n, "the value rectangle of a query batch") ||
	    (want_hits && (!d_hits.alloc(who, 3 * sizeof(int32_t) * (size_t)nqb * (size_t)k, "the hits of a query batch") ||
			   !d_part.alloc(who, part_bytes, "the partial hit lists"))))
		return false;
	struct Sync { /* the stream is drained before the buffers above are freed (declared last) */
		hipStream_t s = nullptr;
		hipEvent_t ev[5] = {}; /* start, range aligned, rows moved (the quantity begins), values done, hits taken */
		~Sync()
		{
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
			for (hipEvent_t e : ev)
				if (e)
					(void)hipEventDestroy(e);
		}
	} sy;
	SA_HIP_CHECK(hipStreamCreateWithFlags(&sy.s, hipStreamNonBlocking), return false);
	for (hipEvent_t &e : sy.ev)
		SA_HIP_CHECK(hipEventCreate(&e), return false);
	std::vector<int32_t> h_den(norm && norm->denominators ? (size_t)(n + m) : 0);
	double seconds = 0.0, t_align = 0.0, t_gather = 0.0, t_hits = 0.0;
	int32_t batches = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = (int32_t)std::min<int64_t>(nqb, m - q0);
		const size_t hits = (size_t)nq * (size_t)k, cap = (size_t)nqb * (size_t)k, elems = (size_t)nq * (size_t)n;
		int32_t *const dr = static_cast<int32_t *>(d_rect.p), *const dv = static_cast<int32_t *>(d_vrect.p);
		int32_t *const di = static_cast<int32_t *>(d_hits.p), *const dval = di ? di + cap : nullptr, *const dsc = di ? di + 2 * cap : nullptr;
		SA_HIP_CHECK(hipEventRecord(sy.ev[0], sy.s), return false);
		if (norm) {
			if (sa_search_range_launch(ctx, (int32_t)q0, nq, dr, d_scratch.p, sy.s, sy.ev[1]) != 0)
				return false;
			SA_HIP_CHECK(hipEventRecord(sy.ev[2], sy.s), return false);
			if (q0 == 0) { /* once per call */
				SA_HIP_CHECK(sa_denominators_launch(ctx, norm->source, static_cast<int32_t *>(d_den.p), sy.s), return false);
			}
			if (normalize_rect_launch(dr, (int32_t)n, (int32_t)q0, nq, static_cast<const int32_t *>(d_den.p), norm->rule, dv, sy.s) != 0)
				return false;
		} else {
			const struct sa_identity_out out = { dr, nullptr, nullptr, dv, denom };
			SA_HIP_CHECK(hipEventRecord(sy.ev[1], sy.s), return false);
			SA_HIP_CHECK(hipEventRecord(sy.ev[2], sy.s), return false);
			if (!sa_identity_rect(who, ctx, (int32_t)q0, nq, &out, sy.s))
				return false;
		}
		SA_HIP_CHECK(hipEventRecord(sy.ev[3], sy.s), return false);
		if (want_hits && (sa_hits_launch(dv, (int32_t)n, nq, k, di, dval, d_part.p, sy.s) != 0 || take_launch(dr, (int32_t)n, nq, k, di, dsc, sy.s) != 0))
			return false;
		SA_HIP_CHECK(hipEventRecord(sy.ev[4], sy.s), return false);
		if (want_hits) {
			SA_HIP_CHECK(hipMemcpyAsync(w.index + q0 * k, di, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, sy.s), return false);
			if (w.value) {
				SA_HIP_CHECK(hipMemcpyAsync(w.value + q0 * k, dval, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, sy.s), return false);
			}
			if (w.score) {
				SA_HIP_CHECK(hipMemcpyAsync(w.score + q0 * k, dsc, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, sy.s), return false);
			}
		}
		if (w.rect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.rect + q0 * n, dr, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return false);
		}
		if (w.vrect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.vrect + q0 * n, dv, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return false);
		}
		if (q0 == 0 && !h_den.empty()) {
			SA_HIP_CHECK(hipMemcpyAsync(h_den.data(), d_den.p, sizeof(int32_t) * h_den.size(), hipMemcpyDeviceToHost, sy.s), return false);
		}
		SA_HIP_CHECK(hipStreamSynchronize(sy.s), return false); /* (the next batch reuses the buffers) */
		float ms[4] = {};
		for (int t = 0; t < 4; t++)
			SA_HIP_CHECK(hipEventElapsedTime(&ms[t], sy.ev[t], sy.ev[t + 1]), return false);
		t_align += (double)ms[0] * 1e-3;
		t_gather += (double)ms[1] * 1e-3;
		seconds += (double)ms[2] * 1e-3;
		t_hits += (double)ms[3] * 1e-3;
		batches++;
	}
	if (!h_den.empty())
		std::copy(h_den.begin(), h_den.end(), norm->denominators);
	g_last_quantity_seconds.store(seconds);
	/* (under percent identity the sweep is the alignment as well: it is what delivers the scores) */
	sa_search_last_set(norm ? t_align : seconds, t_gather, t_hits, batches);
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

/* for sa_search_above.hip (sa_ctx.h) */
int sa_normalize_rect_launch(const int32_t *d_rect, int32_t n_db, int32_t q0, int32_t nq, const int32_t *d_den, int32_t rule, int32_t *d_out,
			     hipStream_t s)
{
	return normalize_rect_launch(d_rect, n_db, q0, nq, d_den, rule, d_out, s);
}
void sa_search_quantity_last_set(double seconds) { g_last_quantity_seconds.store(seconds); }
/* for sa_strands.hip (sa_ctx.h) */
int sa_hits_take_launch(const int32_t *d_rect, int32_t n_db, int32_t nq, int32_t k, const int32_t *d_index, int32_t *d_out, hipStream_t s)
{
	return take_launch(d_rect, n_db, nq, k, d_index, d_out, s);
}

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
		return normalize_rect_launch(d_rect, ctx->search_db, q0, nq, d_den, rule, d_out, (hipStream_t)stream);
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
		return take_launch(d_rect, ctx->search_db, nq, k, d_index, d_out, (hipStream_t)stream);
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
