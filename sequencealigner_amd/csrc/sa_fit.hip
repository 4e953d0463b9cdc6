/*
 * sa_fit.hip -- queries fitted inside database sequences: the whole query against the best substring of the database sequence, the
 * database's overhang free (sa_ctx_fit_rect, sa_ctx_fit_pairs, sa_hip_search_fit; the contract is in include/seqalign_hip.h,
 * "queries fitted inside database sequences").  No reference counterpart.  The payload, the end-cell rule and the walk step are
 * in sa_fit_core.h, which the host compiles as well; every decision is the record of sa_traceback_core.h, so the tie rule exists
 * once.
 *
 *   sa_k_fit<METHOD>  one pair per wavefront: the sweep of sa_k_identity (sa_identity.hip) -- lane l owns column 64 s + l + 1 of
 *                     the QUERY, the database residues enter as rows and travel one lane per step, the strip's last column is
 *                     parked in the context's boundary scratch -- with these differences: lane 0 of strip 0 feeds M[r][0] = 0
 *                     with the payload (0, 0, r); the payload has a third word, the row the path began in, which travels with
 *                     the DPP moves and sits beside the boundary columns in a context-owned buffer of its own (identities and
 *                     columns share the identity sweep's: one 8-byte and one 4-byte load per state and step, each straight into
 *                     its registers -- a 12-byte struct cost a wait of its own in every step behind strip 0); the lane that
 *                     owns column n keeps the end cell (M descending, r ascending: rows arrive in ascending order, so it is
 *                     replaced on strictly greater only), starting from row 0's (border(n), payload (0, n, 0)), and one __shfl
 *                     from lane (n - 1) & 63 broadcasts it.  Lane 0 stores whichever outputs are asked for.
 *                     Two item mappings, by argument: the rectangle (item w = (q - q0) N + d, as sa_sq_identity_item maps it)
 *                     and the list (item w = the pair (d_db[w], N + d_query[w]) from device index arrays).
 * No state is shared between wavefronts: the same input gives the same bytes.
 */
#include <algorithm>
#include <atomic>

#include "sa_search_run.h"
#include "sa_fit_core.h"
#include "sa_search_quantity_core.h"

namespace {

constexpr int32_t SCORE_MIN = INT32_MIN / 2; /* reference src/bio/align.h:19 */
static_assert(SA_ID_SCORE_MIN == SA_SCORE_MIN, "sa_identity_core.h and seqalign_hip.h disagree");

struct FitArgs {
	SaSeqStore st;
	const int32_t *sub; /* s32[24 * 24] */
	int32_t gap_pen, gap_opn, gap_ext;
	int64_t count;                           /* items */
	int32_t n_db, n_queries;                 /* N and the context's query rows */
	int32_t q0;                              /* rectangle: the first query */
	const int32_t *list_query, *list_db;     /* list: [count] each; both null: the rectangle */
	int32_t *score, *db_begin, *db_end, *identities, *columns, *pid; /* [count] each, any of them null */
	int32_t denom;                           /* SA_PID_*, read iff pid */
	int32_t *bnd;                            /* per-wave strip boundary columns (M and X): the context's */
	int64_t bnd_stride;                      /* ints per wave = 2 * (max_len + 2) */
	sa_id_pay *pbnd;                         /* identities and columns of their payloads (PM and PX): bnd_stride pairs per wave */
	int32_t *bbnd;                           /* the third payload word, begin, of PM and PX: bnd_stride ints per wave */
};

__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

/* value shifted in from lane - 1 (DPP wave_shr:1, bound_ctrl off: lane 0 keeps its own and overrides it afterwards) */
__device__ __forceinline__ int32_t from_left(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ sa_fit_pay from_left(sa_fit_pay p)
{
	return sa_fit_make(from_left(p.identities), from_left(p.columns), from_left(p.begin));
}

template <int METHOD>
__global__ __launch_bounds__(256) void sa_k_fit(FitArgs A)
{
	static_assert(METHOD == SA_METHOD_NW || METHOD == SA_METHOD_GA, "fit is defined for NW and Gotoh");
	__shared__ int32_t s_sub[SA_SUB_DIM * SA_SUB_DIM];
	for (int k = threadIdx.x; k < SA_SUB_DIM * SA_SUB_DIM; k += blockDim.x)
		s_sub[k] = A.sub[k];
	__syncthreads();

	const int lane = threadIdx.x & 63;
	const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
	int32_t *bndM = A.bnd + wave * A.bnd_stride;
	int32_t *bndX = bndM + (A.bnd_stride >> 1);
	sa_id_pay *bndPM = A.pbnd + wave * A.bnd_stride;
	sa_id_pay *bndPX = bndPM + (A.bnd_stride >> 1);
	int32_t *bndBM = A.bbnd + wave * A.bnd_stride;
	int32_t *bndBX = bndBM + (A.bnd_stride >> 1);

	const int32_t g = A.gap_pen, o = A.gap_opn, e = A.gap_ext;
	auto border = [&](int32_t k) -> int32_t { return sa_fit_border(METHOD, k, g, o, e); };

	for (int64_t w = wave; w < A.count; w += nwaves) {
		int32_t i, j; /* rows: database sequence i; columns: query j (store index) */
		if (A.list_db) {
			const int32_t d = A.list_db[w], q = A.list_query[w];
			if (d < 0 || d >= A.n_db || q < 0 || q >= A.n_queries) { /* (wave-uniform) nothing is read for it */
				if (lane == 0) {
					if (A.score)
						A.score[w] = INT32_MIN;
					if (A.db_begin)
						A.db_begin[w] = INT32_MIN;
					if (A.db_end)
						A.db_end[w] = INT32_MIN;
					if (A.identities)
						A.identities[w] = INT32_MIN;
					if (A.columns)
						A.columns[w] = INT32_MIN;
					if (A.pid)
						A.pid[w] = INT32_MIN;
				}
				continue;
			}
			i = d;
			j = A.n_db + q;
		} else {
			sa_sq_identity_item(A.n_db, A.q0, w, &i, &j);
		}
		const int32_t m = A.st.meta[i].len, offi = A.st.meta[i].off;
		const int32_t n = A.st.meta[j].len, offj = A.st.meta[j].off;
		const uint8_t *ci = A.st.codes + offi;
		const uint8_t *cj = A.st.codes + offj;
		const int32_t nstrips = (n + 63) >> 6;
		/* the end cell, kept by the lane that owns column n: row 0's to begin with */
		int32_t best = border(n), best_r = 0;
		sa_fit_pay best_p = sa_fit_border_row0(n);
		int32_t h = 0;
		sa_fit_pay pm = sa_fit_make(0, 0, 0);

		for (int32_t s = 0; s < nstrips; s++) {
			const int32_t c = (s << 6) + lane + 1;
			const bool colvalid = c <= n;
			const bool endcol = c == n;
			const int32_t b = colvalid ? cj[c - 1] : 0;
			const int32_t width = (n - (s << 6)) < 64 ? (n - (s << 6)) : 64;
			const bool last_strip = s + 1 == nstrips;
			h = border(c);              /* M[0][c]  */
			pm = sa_fit_border_row0(c); /* PM[0][c] */
			int32_t y = SCORE_MIN;
			sa_fit_pay py = pm;
			int32_t x = SCORE_MIN;
			sa_fit_pay px = pm;
			int32_t diag = border(c - 1); /* (lane 0 of strip 0: border(0) = 0 = M[0][0]) */
			sa_fit_pay dpm = sa_fit_border_row0(c - 1);
			const int32_t steps = m + width - 1;

			for (int32_t t = 0; t < steps; t++) {
				const int32_t r = t - lane + 1;
				/* the residue of this step is asked for before lane 0 asks for the boundary column: one wait covers both */
				const bool valid = colvalid && r >= 1 && r <= m;
				const int32_t a = valid ? ci[r - 1] : 0;
				int32_t lm = from_left(h);
				sa_fit_pay lpm = from_left(pm);
				int32_t lx = SCORE_MIN;
				sa_fit_pay lpx = lpm;
				if (METHOD != SA_METHOD_NW) {
					lx = from_left(x);
					lpx = from_left(px);
				}
				if (lane == 0) {
					if (s == 0) {
						lm = 0; /* M[r][0]: the database's first residues are free */
						lx = SCORE_MIN;
						lpm = lpx = sa_fit_border_col0(r);
					} else if (r <= m) { /* (r >= 1 in lane 0; the boundary arrays hold max_len + 2 entries) */
						lm = bndM[r];
						lpm = sa_fit_make(bndPM[r].identities, bndPM[r].columns, bndBM[r]);
						if (METHOD != SA_METHOD_NW) {
							lx = bndX[r];
							lpx = sa_fit_make(bndPX[r].identities, bndPX[r].columns, bndBX[r]);
						}
					}
				}
				const bool equal = a == b;
				int32_t nm, nx = SCORE_MIN, ny = SCORE_MIN;
				sa_fit_pay npm, npx = px, npy = py;
				if (METHOD == SA_METHOD_NW) {
					const int32_t match = diag + s_sub[a * SA_SUB_DIM + b];
					const int32_t del = h + g;
					const int32_t ins = lm + g;
					nm = imax(ins, imax(del, match));
					npm = sa_fit_step_nw(sa_tb_encode_nw(nm, match, del), equal, dpm, pm, lpm);
				} else {
					const int32_t sd = diag + s_sub[b * SA_SUB_DIM + a];
					const int32_t xo = lm + o, yo = h + o;
					nx = imax(xo, lx + e);
					ny = imax(yo, y + e);
					nm = imax(nx, sd);
					nm = imax(ny, nm);
					const uint32_t rec = sa_tb_encode_affine(false, nm, sd, nx, ny, xo, yo);
					npx = sa_fit_step_x(rec, lpm, lpx);
					npy = sa_fit_step_y(rec, pm, py);
					npm = sa_fit_step_m(rec, equal, dpm, npx, npy);
				}
				diag = lm;
				dpm = lpm;
				if (valid) {
					h = nm;
					x = nx;
					y = ny;
					pm = npm;
					px = npx;
					py = npy;
					if (endcol && nm > best) { /* (rows arrive in ascending order: strictly greater only) */
						best = nm;
						best_r = r;
						best_p = npm;
					}
					if (lane == 63 && !last_strip) {
						bndM[r] = nm;
						bndPM[r] = sa_id_make(npm.identities, npm.columns);
						bndBM[r] = npm.begin;
						if (METHOD != SA_METHOD_NW) {
							bndX[r] = nx;
							bndPX[r] = sa_id_make(npx.identities, npx.columns);
							bndBX[r] = npx.begin;
						}
					}
				}
			}
			if (!last_strip)
				__threadfence_block(); /* boundary column visible to this wave's next strip */
		}

		const int src = (n - 1) & 63; /* the lane that owns column n */
		const int32_t score = __shfl(best, src, 64), db_end = __shfl(best_r, src, 64);
		const sa_fit_pay res = sa_fit_make(__shfl(best_p.identities, src, 64), __shfl(best_p.columns, src, 64), __shfl(best_p.begin, src, 64));
		if (lane == 0) {
			if (A.score)
				A.score[w] = score;
			if (A.db_begin)
				A.db_begin[w] = res.begin;
			if (A.db_end)
				A.db_end[w] = db_end;
			if (A.identities)
				A.identities[w] = res.identities;
			if (A.columns)
				A.columns[w] = res.columns;
			if (A.pid)
				A.pid[w] = sa_id_pid(res.identities, res.columns, m, n, A.denom);
		}
	}
}

/* hits [0, count) of a batch whose first query is q0: the query of hit t is q0 + t / k */
__global__ __launch_bounds__(256) void sa_k_fit_hit_queries(int32_t q0, int32_t k, int64_t count, int32_t *out)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t < count)
		out[t] = q0 + (int32_t)(t / k);
}

std::atomic<double> g_last_fit_seconds{ 0.0 };

/* the boundary payloads: identities and columns beside the identity sweep's, in the buffer the two share (sa_ctx::d_id_scratch);
 * the third word in a buffer of its own, one int per int of d_scratch, allocated when the first fit call of the context comes */
bool fit_scratch(const char *who, sa_ctx *ctx)
{
	if (!sa_identity_payload_scratch(ctx))
		return false;
	if (ctx->d_fit_scratch)
		return true;
	const size_t bytes = (size_t)ctx->generic_blocks * 4 * (size_t)ctx->scratch_stride * sizeof(int32_t);
	if (hipMalloc(&ctx->d_fit_scratch, bytes) != hipSuccess) {
		(void)hipGetLastError();
		ctx->d_fit_scratch = nullptr;
		sa_set_error("%s: %.2f GiB of device memory for the strip-boundary payloads cannot be allocated", who, (double)bytes / (double)(1 << 30));
		return false;
	}
	return true;
}

/* what every fit call refuses about its context and its outputs (no device is touched) */
bool fit_check(const char *who, const sa_ctx *ctx, const struct sa_fit_out *o)
{
	if (!sa_search_ctx_check(who, ctx))
		return false;
	if (ctx->sc.method != SA_METHOD_NW && ctx->sc.method != SA_METHOD_GA) {
		sa_set_error("%s: the context's method is SW, which is local already; fit is defined for NW and Gotoh", who);
		return false;
	}
	if (!o) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (!o->score && !o->db_begin && !o->db_end && !o->identities && !o->columns && !o->pid) {
		sa_set_error("%s: every output is null, nothing to compute", who);
		return false;
	}
	if (o->pid && !sa_identity_denom_check(who, o->denom))
		return false;
	if ((uintptr_t)o->score % 4 || (uintptr_t)o->db_begin % 4 || (uintptr_t)o->db_end % 4 || (uintptr_t)o->identities % 4 || (uintptr_t)o->columns % 4 ||
	    (uintptr_t)o->pid % 4) {
		sa_set_error("%s: the outputs want 4-byte alignment", who);
		return false;
	}
	return true;
}

/* the current device is the context's; everything has been checked.  list_db == nullptr: the rectangle of queries [q0, ...) */
bool launch_fit(const char *who, sa_ctx *ctx, int32_t q0, const int32_t *list_query, const int32_t *list_db, int64_t count, const struct sa_fit_out &out,
		hipStream_t s)
{
	if (count == 0)
		return true;
	if (!fit_scratch(who, ctx))
		return false;
	FitArgs a{};
	a.st.codes = ctx->d_codes;
	a.st.meta = ctx->d_meta;
	a.st.num = ctx->num;
	a.sub = ctx->d_sub;
	a.gap_pen = ctx->sc.gap_pen;
	a.gap_opn = ctx->sc.gap_opn;
	a.gap_ext = ctx->sc.gap_ext;
	a.count = count;
	a.n_db = ctx->search_db;
	a.n_queries = ctx->search_queries;
	a.q0 = q0;
	a.list_query = list_query;
	a.list_db = list_db;
	a.score = out.score;
	a.db_begin = out.db_begin;
	a.db_end = out.db_end;
	a.identities = out.identities;
	a.columns = out.columns;
	a.pid = out.pid;
	a.denom = out.pid ? out.denom : 0;
	a.bnd = ctx->d_scratch;
	a.bnd_stride = ctx->scratch_stride;
	a.pbnd = static_cast<sa_id_pay *>(ctx->d_id_scratch);
	a.bbnd = static_cast<int32_t *>(ctx->d_fit_scratch);
	/* four waves per workgroup, a wave's boundary lines per resident wave: never more workgroups than the context sized them for */
	const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->generic_blocks, (count + 3) / 4));
	if (ctx->sc.method == SA_METHOD_NW)
		hipLaunchKernelGGL(sa_k_fit<SA_METHOD_NW>, dim3(blocks), dim3(256), 0, s, a);
	else
		hipLaunchKernelGGL(sa_k_fit<SA_METHOD_GA>, dim3(blocks), dim3(256), 0, s, a);
	SA_HIP_CHECK(hipGetLastError(), return false);
	return true;
}

int fit_rect_impl(sa_ctx *ctx, int32_t q0, int32_t nq, const struct sa_fit_out *d_out, void *stream)
{
	const char *who = "sa_ctx_fit_rect";
	if (!fit_check(who, ctx, d_out) || !sa_search_queries_check(who, ctx, q0, nq))
		return 1;
	SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
	return launch_fit(who, ctx, q0, nullptr, nullptr, (int64_t)nq * ctx->search_db, *d_out, (hipStream_t)stream) ? 0 : 1;
}

int fit_pairs_impl(sa_ctx *ctx, const int32_t *d_query, const int32_t *d_db, int64_t npairs, const struct sa_fit_out *d_out, void *stream)
{
	const char *who = "sa_ctx_fit_pairs";
	if (!fit_check(who, ctx, d_out))
		return 1;
	if (npairs < 0) {
		sa_set_error("%s: npairs = %lld", who, (long long)npairs);
		return 1;
	}
	if (npairs > 0 && (!d_query || !d_db)) {
		sa_set_error("%s: null index array", who);
		return 1;
	}
	if ((uintptr_t)d_query % 4 || (uintptr_t)d_db % 4) {
		sa_set_error("%s: d_query and d_db want 4-byte alignment", who);
		return 1;
	}
	SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
	return launch_fit(who, ctx, 0, d_query, d_db, npairs, *d_out, (hipStream_t)stream) ? 0 : 1;
}

bool search_fit_impl(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t denom, int32_t *index, int32_t *value,
		     int32_t *score, int32_t *db_begin, int32_t *db_end, int32_t *rect, int32_t *vrect)
{
	const char *who = "sa_hip_search_fit";
	if (!sc) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (sc->method != SA_METHOD_NW && sc->method != SA_METHOD_GA) {
		sa_set_error("%s: method %d: SW is local already; fit is defined for NW and Gotoh", who, sc->method);
		return false;
	}
	const bool want_hits = index || value || score || db_begin || db_end;
	if (want_hits && !index) {
		sa_set_error("%s: value, score, db_begin and db_end belong to the hits of index, which is null", who);
		return false;
	}
	if (!want_hits && !rect && !vrect) {
		sa_set_error("%s: nothing asked for (index, rect and vrect are all null)", who);
		return false;
	}
	if (!sa_run_stores_not_empty(who, db, queries) || !sa_run_stores_not_null(who, db, queries))
		return false;
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	const bool by_pid = denom != -1;
	if (by_pid && !sa_identity_denom_check(who, denom))
		return false;
	if (!sa_run_device_check())
		return false;
	SearchRun run(who);
	if (!run.adopt(sa_ctx_create_search(0, db, queries, sc), db, queries))
		return false;
	sa_ctx *ctx = run.ctx;
	SA_HIP_CHECK(hipSetDevice(ctx->device), return false);
	if (!fit_scratch(who, ctx) || !run.size(sa_batch_per_query_fit(run.n, want_hits, k))) /* (the scratch: before the free memory is read) */
		return false;
	const int32_t n = (int32_t)run.n;
	const size_t rect_bytes = sizeof(int32_t) * (size_t)run.nqb * (size_t)n, cap = (size_t)run.nqb * (size_t)k;
	int32_t *dr = nullptr, *dvr = nullptr, *di = nullptr;
	void *d_part = nullptr;
	if (!run.alloc(dr, rect_bytes, "the rectangle of a query batch") || (by_pid && !run.alloc(dvr, rect_bytes, "the value rectangle of a query batch")) ||
	    (want_hits && (!run.alloc(di, 6 * sizeof(int32_t) * cap, "the hits of a query batch") ||
			   !run.alloc(d_part, run.largest([&](int32_t, int32_t nq) { return sa_hits_scratch_bytes(n, nq, k); }), "the partial hit lists"))))
		return false;
	int32_t *const dv = by_pid ? dvr : dr;
	int32_t *const dval = di ? di + cap : nullptr, *const dsc = di ? di + 2 * cap : nullptr, *const dbeg = di ? di + 3 * cap : nullptr,
		       *const dend = di ? di + 4 * cap : nullptr, *const dqy = di ? di + 5 * cap : nullptr;
	if (!run.start())
		return false;
	const bool ok = run.each_batch([&](int64_t q0, int32_t nq) {
		hipStream_t s = run.sy.s;
		const size_t hits = (size_t)nq * (size_t)k, elems = (size_t)nq * (size_t)n;
		const struct sa_fit_out sweep = { dr, nullptr, nullptr, nullptr, nullptr, by_pid ? dv : nullptr, by_pid ? denom : 0 };
		if (!run.stamp(SA_PH_FIT) || !launch_fit(who, ctx, (int32_t)q0, nullptr, nullptr, (int64_t)elems, sweep, s))
			return false;
		if (want_hits) {
			if (!run.stamp(SA_PH_SELECT) || sa_hits_launch(dv, n, nq, k, di, dval, d_part, s) != 0)
				return false;
			hipLaunchKernelGGL(sa_k_fit_hit_queries, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, s, (int32_t)q0, k, (int64_t)hits, dqy);
			SA_HIP_CHECK(hipGetLastError(), return false);
			const struct sa_fit_out list = { dsc, dbeg, dend, nullptr, nullptr, nullptr, 0 };
			if (!run.stamp(SA_PH_FIT) || !launch_fit(who, ctx, 0, dqy, di, (int64_t)hits, list, s))
				return false;
		}
		if (!run.stamp(SA_PH_END))
			return false;
		if (want_hits) {
			int32_t *const host[5] = { index, value, score, db_begin, db_end };
			const int32_t *const dev[5] = { di, dval, dsc, dbeg, dend };
			for (int t = 0; t < 5; t++)
				if (host[t]) {
					SA_HIP_CHECK(hipMemcpyAsync(host[t] + q0 * k, dev[t], sizeof(int32_t) * hits, hipMemcpyDeviceToHost, s), return false);
				}
		}
		if (rect) {
			SA_HIP_CHECK(hipMemcpyAsync(rect + q0 * n, dr, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
		}
		if (vrect) {
			SA_HIP_CHECK(hipMemcpyAsync(vrect + q0 * n, dv, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
		}
		return true;
	});
	if (!ok)
		return false;
	const PhaseClock &t = run.sy.clock;
	g_last_fit_seconds.store(t[SA_PH_FIT]);
	sa_search_last_set(t[SA_PH_FIT], 0.0, t[SA_PH_SELECT], run.batches); /* (the sweep is the alignment: it is what delivers the scores) */
	return true;
}

} // namespace

extern "C" int sa_ctx_fit_rect(sa_ctx *ctx, int32_t q0, int32_t nq, const struct sa_fit_out *d_out, void *stream)
{
	return sa_guard("sa_ctx_fit_rect", 1, [&] { return fit_rect_impl(ctx, q0, nq, d_out, stream); });
}

extern "C" int sa_ctx_fit_pairs(sa_ctx *ctx, const int32_t *d_query, const int32_t *d_db, int64_t npairs, const struct sa_fit_out *d_out, void *stream)
{
	return sa_guard("sa_ctx_fit_pairs", 1, [&] { return fit_pairs_impl(ctx, d_query, d_db, npairs, d_out, stream); });
}

extern "C" bool sa_hip_search_fit(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, int32_t k, int32_t denom, int32_t *index,
				  int32_t *value, int32_t *score, int32_t *db_begin, int32_t *db_end, int32_t *rect, int32_t *vrect)
{
	return sa_guard("sa_hip_search_fit", false,
			[&] { return search_fit_impl(db, queries, sc, k, denom, index, value, score, db_begin, db_end, rect, vrect); });
}

extern "C" double sa_hip_last_search_fit_seconds(void)
{
	return sa_guard("sa_hip_last_search_fit_seconds", 0.0, [&] { return g_last_fit_seconds.load(); });
}
