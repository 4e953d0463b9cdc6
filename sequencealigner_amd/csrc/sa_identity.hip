/*
 * sa_identity.hip -- percent identity of every pair: identities and columns of the canonical alignment of the alignment contract
 * (include/seqalign_hip.h), carried forward through the DP sweep instead of recorded and walked back (sa_ctx_identity_range,
 * sa_hip_identity, sa_pid_value, and the in-place sweep behind sa_zjob_identity and the *_pid one-call selections).  No reference
 * counterpart: the reference keeps scores only.  The payload and its update rules are in sa_identity_core.h, which the host
 * compiles as well; every decision is the record of sa_traceback_core.h, so the tie rule exists once.
 *
 *   sa_k_identity<METHOD>  one pair per wavefront: the sweep of sa_k_trace_fill (sa_traceback.hip) without the decision stores --
 *                          lane l owns column 64 s + l + 1, rows travel one lane per step, the strip's last column is parked in
 *                          the context's boundary scratch.  Every lane keeps a payload (identities, columns) per state; the left
 *                          and diagonal payloads travel with the DPP move next to their scores; the last column's PM (and PX)
 *                          sit beside bndM / bndX in a context-owned buffer of their own.  SW keeps the payload of its lane's end
 *                          cell and reduces it with the end key (best descending, r ascending, c ascending).  Lane 0 stores
 *                          whichever of score / identities / columns / pid are asked for at [p - start]; pid is computed from
 *                          the two lengths in the kernel, so a triangle of scores can be overwritten in place.
 *                          RECT = true is the rectangle form of a search context (sa_ctx_identity_rect): wave item q is element q
 *                          of the dense outputs and the pair (d, N + q0 + r), q = r N + d -- that mapping is the only difference,
 *                          the body is the one body.
 * No state is shared between wavefronts: the same input gives the same bytes.
 */
#include <algorithm>
#include <atomic>

#include "sa_ctx.h"
#include "sa_identity_core.h"
#include "sa_search_quantity_core.h"

static_assert(SA_ID_DENOM_COLUMNS == SA_PID_COLUMNS && SA_ID_DENOM_SHORTER == SA_PID_SHORTER && SA_ID_DENOM_LONGER == SA_PID_LONGER &&
		      SA_ID_DENOM_MEAN == SA_PID_MEAN,
	      "sa_identity_core.h and seqalign_hip.h disagree");
static_assert(SA_ID_PPM == SA_NORM_SCALE && SA_ID_SCORE_MIN == SA_SCORE_MIN, "sa_identity_core.h and seqalign_hip.h disagree");
static_assert(SA_TB_NW == SA_METHOD_NW && SA_TB_GA == SA_METHOD_GA && SA_TB_SW == SA_METHOD_SW, "sa_traceback_core.h and seqalign_hip.h disagree");

namespace {

constexpr int32_t SCORE_MIN = INT32_MIN / 2; /* reference src/bio/align.h:19 */

struct IdArgs {
	SaSeqStore st;
	const int32_t *sub; /* s32[24 * 24] */
	int32_t gap_pen, gap_opn, gap_ext;
	int64_t start, count;                          /* packed pair range */
	int32_t *score, *identities, *columns, *pid;   /* [count] each, any of them null */
	int32_t denom;                                 /* SA_PID_*, read iff pid */
	int32_t rect_n;                                /* RECT: the database size N; start is then the first query q0 (in the padding before bnd) */
	int32_t *bnd;                                  /* per-wave strip boundary columns (M and X): the context's */
	int64_t bnd_stride;                            /* ints per wave = 2 * (max_len + 2) */
	sa_id_pay *pbnd;                               /* their payloads (PM and PX): bnd_stride payloads per wave */
};

__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

/* packed index -> (i, j), i < j: largest j with j (j - 1) / 2 <= p, as sa_k_pair_per_wave does it */
__device__ __forceinline__ void unpack_pair(int64_t p, int32_t &i, int32_t &j)
{
	int64_t jj = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
	while (jj * (jj - 1) / 2 > p)
		--jj;
	while ((jj + 1) * jj / 2 <= p)
		++jj;
	j = (int32_t)jj;
	i = (int32_t)(p - jj * (jj - 1) / 2);
}

/* value shifted in from lane - 1 (DPP wave_shr:1, bound_ctrl off: lane 0 keeps its own and overrides it afterwards) */
__device__ __forceinline__ int32_t from_left(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ sa_id_pay from_left(sa_id_pay p) { return sa_id_make(from_left(p.identities), from_left(p.columns)); }

__device__ __forceinline__ sa_id_pay shfl_xor(sa_id_pay p, int d) { return sa_id_make(__shfl_xor(p.identities, d, 64), __shfl_xor(p.columns, d, 64)); }

template <int METHOD, bool RECT>
__global__ __launch_bounds__(256) void sa_k_identity(IdArgs A)
{
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

	const int32_t g = A.gap_pen, o = A.gap_opn, e = A.gap_ext;
	/* closed forms of the reference's borders, as in sa_k_pair_per_wave */
	const int32_t ga_b1 = imax(o, SCORE_MIN + e);
	const int32_t ga_w = imax(o, e);
	auto border = [&](int32_t k) -> int32_t {
		if (METHOD == SA_METHOD_NW)
			return k * g;
		if (METHOD == SA_METHOD_GA)
			return k == 0 ? 0 : ga_b1 + (k - 1) * ga_w;
		return 0;
	};

	for (int64_t q = wave; q < A.count; q += nwaves) {
		int32_t i, j;
		if (RECT)
			sa_sq_identity_item(A.rect_n, (int32_t)A.start, q, &i, &j);
		else
			unpack_pair(A.start + q, i, j);
		const int32_t m = A.st.meta[i].len, offi = A.st.meta[i].off; /* rows: seq i    */
		const int32_t n = A.st.meta[j].len, offj = A.st.meta[j].off; /* columns: seq j */
		const uint8_t *ci = A.st.codes + offi;
		const uint8_t *cj = A.st.codes + offj;
		const int32_t nstrips = (n + 63) >> 6;
		int32_t best = 0, best_r = 0, best_c = 0; /* SW end cell of this lane ... */
		sa_id_pay best_p = sa_id_make(0, 0);     /* ... and PM there             */
		int32_t h = 0;
		sa_id_pay pm = sa_id_make(0, 0);

		for (int32_t s = 0; s < nstrips; s++) {
			const int32_t c = (s << 6) + lane + 1;
			const bool colvalid = c <= n;
			const int32_t b = colvalid ? cj[c - 1] : 0;
			const int32_t width = (n - (s << 6)) < 64 ? (n - (s << 6)) : 64;
			const bool last_strip = s + 1 == nstrips;
			h = border(c);                 /* M[0][c]  */
			pm = sa_id_border(METHOD, c);  /* PM[0][c] */
			int32_t y = SCORE_MIN;
			sa_id_pay py = sa_id_border(METHOD, c);
			int32_t x = SCORE_MIN;
			sa_id_pay px = sa_id_border(METHOD, c);
			int32_t diag = border(c - 1);
			sa_id_pay dpm = sa_id_border(METHOD, c - 1);
			const int32_t steps = m + width - 1;

			for (int32_t t = 0; t < steps; t++) {
				const int32_t r = t - lane + 1;
				int32_t lm = from_left(h);
				sa_id_pay lpm = from_left(pm);
				int32_t lx = SCORE_MIN;
				sa_id_pay lpx = lpm;
				if (METHOD != SA_METHOD_NW) {
					lx = from_left(x);
					lpx = from_left(px);
				}
				if (lane == 0) {
					if (s == 0) {
						lm = border(r);
						lx = SCORE_MIN;
						lpm = lpx = sa_id_border(METHOD, r);
					} else if (r <= m) { /* (r >= 1 in lane 0; the boundary arrays hold max_len + 2 entries) */
						lm = bndM[r];
						lpm = bndPM[r];
						if (METHOD != SA_METHOD_NW) {
							lx = bndX[r];
							lpx = bndPX[r];
						}
					}
				}
				const bool valid = colvalid && r >= 1 && r <= m;
				const int32_t a = valid ? ci[r - 1] : 0;
				const bool equal = a == b;
				int32_t nm, nx = SCORE_MIN, ny = SCORE_MIN;
				sa_id_pay npm, npx = px, npy = py;
				if (METHOD == SA_METHOD_NW) {
					const int32_t match = diag + s_sub[a * SA_SUB_DIM + b];
					const int32_t del = h + g;
					const int32_t ins = lm + g;
					nm = imax(ins, imax(del, match));
					npm = sa_id_step_nw(sa_tb_encode_nw(nm, match, del), equal, dpm, pm, lpm);
				} else {
					const int32_t sd = diag + s_sub[b * SA_SUB_DIM + a];
					const int32_t xo = lm + o, yo = h + o;
					nx = imax(xo, lx + e);
					ny = imax(yo, y + e);
					nm = (METHOD == SA_METHOD_SW) ? imax(sd, 0) : sd;
					nm = imax(nx, nm);
					nm = imax(ny, nm);
					const uint32_t rec = sa_tb_encode_affine(METHOD == SA_METHOD_SW, nm, sd, nx, ny, xo, yo);
					npx = sa_id_step_x(rec, lpm, lpx);
					npy = sa_id_step_y(rec, pm, py);
					npm = sa_id_step_m(rec, equal, dpm, npx, npy);
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
					if (METHOD == SA_METHOD_SW && sa_tb_end_before(nm, r, c, best, best_r, best_c)) {
						best = nm;
						best_r = r;
						best_c = c;
						best_p = npm;
					}
					if (lane == 63 && !last_strip) {
						bndM[r] = nm;
						bndPM[r] = npm;
						if (METHOD != SA_METHOD_NW) {
							bndX[r] = nx;
							bndPX[r] = npx;
						}
					}
				}
			}
			if (!last_strip)
				__threadfence_block(); /* boundary column visible to this wave's next strip */
		}

		int32_t score;
		sa_id_pay res;
		if (METHOD == SA_METHOD_SW) {
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				const int32_t ov = __shfl_xor(best, d, 64), orr = __shfl_xor(best_r, d, 64), oc = __shfl_xor(best_c, d, 64);
				const sa_id_pay op = shfl_xor(best_p, d);
				if (sa_tb_end_before(ov, orr, oc, best, best_r, best_c)) {
					best = ov;
					best_r = orr;
					best_c = oc;
					best_p = op;
				}
			}
			score = best;
			res = best_p;
		} else {
			const int src = (n - 1) & 63; /* M[m][n] sits in the lane owning column n */
			score = __shfl(h, src, 64);
			res = sa_id_make(__shfl(pm.identities, src, 64), __shfl(pm.columns, src, 64));
		}
		if (lane == 0) {
			if (A.score)
				A.score[q] = score;
			if (A.identities)
				A.identities[q] = res.identities;
			if (A.columns)
				A.columns[q] = res.columns;
			if (A.pid)
				A.pid[q] = sa_id_pid(res.identities, res.columns, m, n, A.denom);
		}
	}
}

std::atomic<double> g_last_identity_seconds{ 0.0 };

bool denom_ok(const char *who, int32_t denom)
{
	if (sa_id_denom_ok(denom))
		return true;
	sa_set_error("%s: denom %d is none of SA_PID_COLUMNS (%d), SA_PID_SHORTER (%d), SA_PID_LONGER (%d), SA_PID_MEAN (%d)", who, denom,
		     (int)SA_PID_COLUMNS, (int)SA_PID_SHORTER, (int)SA_PID_LONGER, (int)SA_PID_MEAN);
	return false;
}

/* the boundary payloads: as many entries as d_scratch has ints, allocated when the first identity call of the context comes */
bool payload_scratch(sa_ctx *ctx)
{
	if (ctx->d_id_scratch)
		return true;
	const size_t bytes = (size_t)ctx->generic_blocks * 4 * (size_t)ctx->scratch_stride * sizeof(sa_id_pay);
	if (hipMalloc(&ctx->d_id_scratch, bytes) != hipSuccess) {
		(void)hipGetLastError();
		ctx->d_id_scratch = nullptr;
		sa_set_error("sa_ctx_identity_range: %.2f GiB of device memory for the strip-boundary payloads cannot be allocated",
			     (double)bytes / (double)(1 << 30));
		return false;
	}
	return true;
}

/* the current device is the context's; the range and the outputs have been checked.  rect_n = 0: the packed range [start,
 * start + count); rect_n = N > 0: the rectangle form, start the first query and count = nq * N */
bool launch_identity(sa_ctx *ctx, int64_t start, int64_t count, const struct sa_identity_out &out, hipStream_t s, int32_t rect_n = 0)
{
	if (count == 0)
		return true;
	if (!payload_scratch(ctx))
		return false;
	IdArgs a{};
	a.st.codes = ctx->d_codes;
	a.st.meta = ctx->d_meta;
	a.st.num = ctx->num;
	a.sub = ctx->d_sub;
	a.gap_pen = ctx->sc.gap_pen;
	a.gap_opn = ctx->sc.gap_opn;
	a.gap_ext = ctx->sc.gap_ext;
	a.start = start;
	a.count = count;
	a.score = out.score;
	a.identities = out.identities;
	a.columns = out.columns;
	a.pid = out.pid;
	a.denom = out.pid ? out.denom : 0;
	a.rect_n = rect_n;
	a.bnd = ctx->d_scratch;
	a.bnd_stride = ctx->scratch_stride;
	a.pbnd = static_cast<sa_id_pay *>(ctx->d_id_scratch);
	/* four waves per workgroup, a wave's boundary lines per resident wave: never more workgroups than the context sized them for */
	const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->generic_blocks, (count + 3) / 4));
	switch (ctx->sc.method) {
	case SA_METHOD_NW:
		if (rect_n)
			hipLaunchKernelGGL((sa_k_identity<SA_METHOD_NW, true>), dim3(blocks), dim3(256), 0, s, a);
		else
			hipLaunchKernelGGL((sa_k_identity<SA_METHOD_NW, false>), dim3(blocks), dim3(256), 0, s, a);
		break;
	case SA_METHOD_GA:
		if (rect_n)
			hipLaunchKernelGGL((sa_k_identity<SA_METHOD_GA, true>), dim3(blocks), dim3(256), 0, s, a);
		else
			hipLaunchKernelGGL((sa_k_identity<SA_METHOD_GA, false>), dim3(blocks), dim3(256), 0, s, a);
		break;
	case SA_METHOD_SW:
		if (rect_n)
			hipLaunchKernelGGL((sa_k_identity<SA_METHOD_SW, true>), dim3(blocks), dim3(256), 0, s, a);
		else
			hipLaunchKernelGGL((sa_k_identity<SA_METHOD_SW, false>), dim3(blocks), dim3(256), 0, s, a);
		break;
	default:
		sa_set_error("sa_ctx_identity_range: method %d", ctx->sc.method);
		return false;
	}
	SA_HIP_CHECK(hipGetLastError(), return false);
	return true;
}

/* what sa_ctx_identity_range and sa_hip_identity refuse about their outputs */
bool outputs_ok(const char *who, const int32_t *score, const int32_t *identities, const int32_t *columns, const int32_t *pid, int32_t denom)
{
	if (!score && !identities && !columns && !pid) {
		sa_set_error("%s: every output is null, nothing to compute", who);
		return false;
	}
	return !pid || denom_ok(who, denom);
}

int identity_range_impl(sa_ctx *ctx, int64_t start, int64_t count, const struct sa_identity_out *d_out, void *stream)
{
	const char *who = "sa_ctx_identity_range";
	if (!ctx || !d_out) {
		sa_set_error("%s: null argument", who);
		return 1;
	}
	if (!outputs_ok(who, d_out->score, d_out->identities, d_out->columns, d_out->pid, d_out->denom))
		return 1;
	if (start < 0 || count < 0 || start > ctx->pairs || count > ctx->pairs - start) {
		sa_set_error("%s: the range [%lld, %lld + %lld) is outside the %lld pairs", who, (long long)start, (long long)start, (long long)count,
			     (long long)ctx->pairs);
		return 1;
	}
	if ((uintptr_t)d_out->score % 4 || (uintptr_t)d_out->identities % 4 || (uintptr_t)d_out->columns % 4 || (uintptr_t)d_out->pid % 4) {
		sa_set_error("%s: the outputs want 4-byte alignment", who);
		return 1;
	}
	SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
	return launch_identity(ctx, start, count, *d_out, (hipStream_t)stream) ? 0 : 1;
}

bool hip_identity_impl(struct sa_input in, const struct sa_scoring *sc, int32_t denom, int32_t *identities, int32_t *columns, int32_t *pid)
{
	const char *who = "sa_hip_identity";
	if (!sc || !in.seqs || !in.meta) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (!outputs_ok(who, nullptr, identities, columns, pid, denom))
		return false;
	if (sa_hip_device_count() <= 0) {
		sa_set_error("No HIP devices available; libseqalign_hip has no CPU fallback");
		return false;
	}
	struct Run { /* (released whatever way the function is left; the stream is drained first) */
		sa_ctx *ctx = nullptr;
		int32_t *d[3] = { nullptr, nullptr, nullptr };
		hipStream_t s = nullptr;
		hipEvent_t e0 = nullptr, e1 = nullptr;
		~Run()
		{
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
			if (e0)
				(void)hipEventDestroy(e0);
			if (e1)
				(void)hipEventDestroy(e1);
			for (int32_t *p : d)
				(void)hipFree(p);
			if (ctx)
				sa_ctx_destroy(ctx);
		}
	} run;
	run.ctx = sa_ctx_create(0, in, sc);
	if (!run.ctx)
		return false;
	sa_ctx *ctx = run.ctx;
	SA_HIP_CHECK(hipSetDevice(ctx->device), return false);
	if (ctx->pairs == 0)
		return true;
	if (!payload_scratch(ctx)) /* (before the free memory is read) */
		return false;
	/* column-aligned ranges: as many whole columns as the buffers of the outputs asked for may hold, at least one */
	int32_t *const host[3] = { identities, columns, pid };
	const int nout = (identities != nullptr) + (columns != nullptr) + (pid != nullptr);
	size_t free_b = 0, total_b = 0;
	SA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b), return false);
	int64_t cap = (int64_t)(free_b / 2);
	if (ctx->env.identity_batch_bytes > 0)
		cap = std::min<int64_t>(cap, ctx->env.identity_batch_bytes);
	const int64_t cap_elems = std::min<int64_t>(ctx->pairs, std::max<int64_t>(cap / (4 * nout), (int64_t)ctx->num - 1));
	for (int k = 0; k < 3; k++)
		if (host[k] && hipMalloc(&run.d[k], sizeof(int32_t) * (size_t)cap_elems) != hipSuccess) {
			(void)hipGetLastError();
			run.d[k] = nullptr;
			sa_set_error("%s: %.2f GiB of device memory for a range of columns cannot be allocated", who, (double)cap_elems * 4.0 / (double)(1 << 30));
			return false;
		}
	SA_HIP_CHECK(hipStreamCreateWithFlags(&run.s, hipStreamNonBlocking), return false);
	SA_HIP_CHECK(hipEventCreate(&run.e0), return false);
	SA_HIP_CHECK(hipEventCreate(&run.e1), return false);
	double seconds = 0.0;
	for (int64_t ja = 1; ja < ctx->num;) {
		int64_t jb = ja + 1; /* columns [ja, jb): the pairs [tri(ja), tri(jb)) */
		while (jb < ctx->num && sa_tri(jb + 1) - sa_tri(ja) <= cap_elems)
			jb++;
		const int64_t start = sa_tri(ja), count = sa_tri(jb) - start;
		struct sa_identity_out out = { nullptr, run.d[0], run.d[1], run.d[2], denom };
		SA_HIP_CHECK(hipEventRecord(run.e0, run.s), return false);
		if (!launch_identity(ctx, start, count, out, run.s))
			return false;
		SA_HIP_CHECK(hipEventRecord(run.e1, run.s), return false);
		for (int k = 0; k < 3; k++)
			if (host[k]) {
				SA_HIP_CHECK(hipMemcpyAsync(host[k] + start, run.d[k], sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, run.s), return false);
			}
		SA_HIP_CHECK(hipStreamSynchronize(run.s), return false);
		float ms = 0.f;
		SA_HIP_CHECK(hipEventElapsedTime(&ms, run.e0, run.e1), return false);
		seconds += (double)ms * 1e-3;
		ja = jb;
	}
	g_last_identity_seconds.store(seconds);
	return true;
}

} // namespace

bool sa_identity_denom_check(const char *who, int32_t denom) { return denom_ok(who, denom); }

/* the context's boundary payloads, allocated now instead of at its first sweep: for a caller that sizes buffers from the free memory */
bool sa_identity_payload_scratch(sa_ctx *ctx) { return payload_scratch(ctx); }

/* the rectangle form on a search context: queries [q0, q0 + nq), element (q - q0) * N + d of every non-null output.  The
 * context, the queries and the stream's device are the caller's to have checked; the outputs are checked here as
 * sa_ctx_identity_range checks them. */
bool sa_identity_rect(const char *who, sa_ctx *ctx, int32_t q0, int32_t nq, const struct sa_identity_out *d_out, hipStream_t s)
{
	if (!d_out) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (!outputs_ok(who, d_out->score, d_out->identities, d_out->columns, d_out->pid, d_out->denom))
		return false;
	if ((uintptr_t)d_out->score % 4 || (uintptr_t)d_out->identities % 4 || (uintptr_t)d_out->columns % 4 || (uintptr_t)d_out->pid % 4) {
		sa_set_error("%s: the outputs want 4-byte alignment", who);
		return false;
	}
	SA_HIP_CHECK(hipSetDevice(ctx->device), return false);
	return launch_identity(ctx, q0, (int64_t)nq * ctx->search_db, *d_out, s, ctx->search_db);
}

/* pid of every pair over a device matrix of ctx's store, in place of whatever it held, in order on `s`, which is synchronised: what
 * sa_zjob_identity and the *_pid one-call selections share.  The current device is the matrix's. */
bool sa_identity_in_place(const char *who, sa_ctx *ctx, int32_t *d_packed, int32_t denom, hipStream_t s)
{
	struct Ev {
		hipEvent_t e[2] = { nullptr, nullptr };
		~Ev()
		{
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
		}
	} t;
	if (!denom_ok(who, denom))
		return false;
	for (hipEvent_t &ev : t.e)
		SA_HIP_CHECK(hipEventCreate(&ev), return false);
	struct sa_identity_out out = { nullptr, nullptr, nullptr, d_packed, denom };
	SA_HIP_CHECK(hipEventRecord(t.e[0], s), return false);
	if (!launch_identity(ctx, 0, ctx->pairs, out, s))
		return false;
	SA_HIP_CHECK(hipEventRecord(t.e[1], s), return false);
	SA_HIP_CHECK(hipStreamSynchronize(s), return false);
	float ms = 0.f;
	SA_HIP_CHECK(hipEventElapsedTime(&ms, t.e[0], t.e[1]), return false);
	g_last_identity_seconds.store((double)ms * 1e-3);
	return true;
}

extern "C" int32_t sa_pid_value(int32_t identities, int32_t columns, int32_t len_i, int32_t len_j, int32_t denom)
{
	return sa_guard("sa_pid_value", (int32_t)INT32_MIN, [&]() -> int32_t {
		if (!denom_ok("sa_pid_value", denom))
			return INT32_MIN;
		return sa_id_pid(identities, columns, len_i, len_j, denom);
	});
}

extern "C" int sa_ctx_identity_range(sa_ctx *ctx, int64_t start, int64_t count, const struct sa_identity_out *d_out, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_identity_range"))
		return 1;
	return sa_guard("sa_ctx_identity_range", 1, [&] { return identity_range_impl(ctx, start, count, d_out, stream); });
}

extern "C" bool sa_hip_identity(struct sa_input in, const struct sa_scoring *sc, int32_t denom, int32_t *identities, int32_t *columns, int32_t *pid)
{
	return sa_guard("sa_hip_identity", false, [&] { return hip_identity_impl(in, sc, denom, identities, columns, pid); });
}

extern "C" double sa_hip_last_identity_seconds(void)
{
	return sa_guard("sa_hip_last_identity_seconds", 0.0, [&] { return g_last_identity_seconds.load(); });
}
