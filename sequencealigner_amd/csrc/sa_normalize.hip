/*
 * sa_normalize.hip -- normalised scores: the per-sequence denominators (self-scores or lengths) and the sweep that divides the
 * device-resident packed triangle by them (sa_ctx_denominators, sa_ctx_normalize, sa_zjob_normalize and the *_norm one-call
 * variants).  No reference counterpart: the reference delivers raw scores, which grow with length, and leaves the division
 * to whoever holds the N x N matrix on the host.  The contract and the arithmetic are in sa_normalize_core.h.
 *
 *   sa_k_self<METHOD>     one wavefront per sequence k: the anti-diagonal s32 sweep of sa_wave_sweep.inc, the one of
 *                         sa_k_pair_per_wave, for the pair (k, k) -- the sequence is the row AND the column sequence, the
 *                         table is indexed as for any pair, the full DP runs (under an asymmetric table, or one whose
 *                         diagonal is not the row maximum, the self-score is not the sum of the diagonal entries).  64-column
 *                         strips through the context's per-wave strip-boundary scratch: any length the store accepts.
 *   sa_k_lengths          d[k] = meta[k].len.
 *   sa_k_normalize<RULE>  one streaming pass, 4 P bytes in and 4 P bytes out.  A workgroup takes units of the deal of
 *                         sa_normalize_core.h -- the columns t and N - 1 - t, N - 1 entries together -- and walks each column's
 *                         contiguous run: d[j] is uniform, d[i] a coalesced load, no packed index is ever inverted.  A run
 *                         starts wherever j (j - 1) / 2 falls: the up to three entries before the first 16-byte boundary and
 *                         after the last go element by element, the body as 16-byte loads and stores (when source and
 *                         destination disagree about where that boundary is, the whole run goes element by element).  Every entry
 *                         is read and written by the same thread, once: in place (d_out == d_packed) is as good as disjoint.
 * Neither kernel shares state between workgroups: the same input gives the same bytes.
 */
#include <algorithm>
#include <atomic>

#include "sa_ctx.h"
#include "sa_normalize_core.h"
#include "sa_wave_sweep.h"

static_assert(SA_NORM_SRC_SELF == SA_NORM_SELF && SA_NORM_SRC_LENGTH == SA_NORM_LENGTH, "sa_normalize_core.h and seqalign_hip.h disagree");
static_assert(SA_NORM_RULE_MIN == SA_NORM_MIN && SA_NORM_RULE_MAX == SA_NORM_MAX && SA_NORM_RULE_MEAN == SA_NORM_MEAN,
	      "sa_normalize_core.h and seqalign_hip.h disagree");
static_assert(SA_NORM_PPM == SA_NORM_SCALE, "sa_normalize_core.h and seqalign_hip.h disagree");

namespace {

constexpr int NORM_THREADS = 256;
constexpr int NORM_WGS_PER_CU = 8;

struct SelfArgs {
	SaSeqStore st;
	const int32_t *sub;     /* s32[24 * 24] */
	int32_t gap_pen, gap_opn, gap_ext;
	int32_t *den;           /* den[k] = score of (k, k) */
	int32_t *scratch;       /* per-wave strip boundary columns (M and X): the context's, as sa_k_pair_per_wave uses it */
	int64_t scratch_stride; /* ints per wave = 2 * (max_len + 2) */
};

/* the pair (k, k): the sequence rides the sweep as its rows and as its columns */
template <int METHOD>
__global__ __launch_bounds__(256) void sa_k_self(SelfArgs A)
{
	__shared__ int32_t s_sub[SA_SUB_DIM * SA_SUB_DIM];
	for (int k = threadIdx.x; k < SA_SUB_DIM * SA_SUB_DIM; k += blockDim.x)
		s_sub[k] = A.sub[k];
	__syncthreads();
	const int lane = threadIdx.x & 63;
	const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
	int32_t *bndM = A.scratch + wave * A.scratch_stride;
	int32_t *bndX = bndM + (A.scratch_stride >> 1);
	const int32_t g = A.gap_pen, o = A.gap_opn, e = A.gap_ext;

	for (int64_t k = wave; k < A.st.num; k += nwaves) {
		const int32_t m = A.st.meta[k].len, n = m; /* rows and columns */
		const uint8_t *ci = A.st.codes + A.st.meta[k].off, *cj = ci;
#include "sa_wave_sweep.inc"
		const int32_t score = METHOD == SA_METHOD_SW ? wave_max(best) : mn;
		if (lane == 0)
			A.den[k] = score;
	}
}

__global__ __launch_bounds__(256) void sa_k_lengths(const sa_meta *__restrict__ meta, int32_t num, int32_t *__restrict__ den)
{
	for (int32_t k = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x); k < num; k += (int32_t)(gridDim.x * blockDim.x))
		den[k] = meta[k].len;
}

typedef int32_t i32x4u __attribute__((ext_vector_type(4), aligned(4))); /* d[i .. i + 4): wherever i falls */

/* column j: in[0 .. j) -> out[0 .. j), the workgroup's threads together.  `in` and `out` may be the same. */
template <int RULE>
__device__ __forceinline__ void norm_column(const int32_t *in, int32_t *out, const int32_t *__restrict__ den, int64_t j)
{
	const int tid = threadIdx.x;
	const int32_t dj = den[j];
	/* entries before the first 16-byte boundary of the run; all of it when source and destination disagree about it */
	int64_t head = (int64_t)(((16 - ((uintptr_t)in & 15)) & 15) / 4);
	if ((((uintptr_t)in ^ (uintptr_t)out) & 15) != 0 || head > j)
		head = j;
	const int64_t vecs = (j - head) / 4;
	for (int64_t i = tid; i < head; i += NORM_THREADS)
		out[i] = sa_norm_value_t<RULE>(in[i], den[i], dj);
	const int4 *vin = reinterpret_cast<const int4 *>(in + head);
	int4 *vout = reinterpret_cast<int4 *>(out + head);
	for (int64_t v = tid; v < vecs; v += 2 * NORM_THREADS) {
		const int64_t v1 = v + NORM_THREADS;
		const bool two = v1 < vecs;
		const int4 s0 = vin[v];
		const i32x4u d0 = *reinterpret_cast<const i32x4u *>(den + head + 4 * v);
		int4 s1 = make_int4(0, 0, 0, 0);
		i32x4u d1 = { 1, 1, 1, 1 };
		if (two) {
			s1 = vin[v1];
			d1 = *reinterpret_cast<const i32x4u *>(den + head + 4 * v1);
		}
		int4 r0, r1;
		r0.x = sa_norm_value_t<RULE>(s0.x, d0.x, dj);
		r0.y = sa_norm_value_t<RULE>(s0.y, d0.y, dj);
		r0.z = sa_norm_value_t<RULE>(s0.z, d0.z, dj);
		r0.w = sa_norm_value_t<RULE>(s0.w, d0.w, dj);
		vout[v] = r0;
		if (two) {
			r1.x = sa_norm_value_t<RULE>(s1.x, d1.x, dj);
			r1.y = sa_norm_value_t<RULE>(s1.y, d1.y, dj);
			r1.z = sa_norm_value_t<RULE>(s1.z, d1.z, dj);
			r1.w = sa_norm_value_t<RULE>(s1.w, d1.w, dj);
			vout[v1] = r1;
		}
	}
	for (int64_t i = head + 4 * vecs + tid; i < j; i += NORM_THREADS)
		out[i] = sa_norm_value_t<RULE>(in[i], den[i], dj);
}

/* (no __restrict__ on packed / out: they may be the same buffer) */
template <int RULE>
__global__ __launch_bounds__(NORM_THREADS) void sa_k_normalize(const int32_t *packed, const int32_t *__restrict__ den, int32_t num, int32_t *out)
{
	const int64_t units = sa_norm_units(num);
	for (int64_t t = blockIdx.x; t < units; t += gridDim.x) { /* (uniform in the workgroup) */
		int64_t a, b;
		sa_norm_deal(num, t, &a, &b);
		if (a > 0) /* (column 0 is empty) */
			norm_column<RULE>(packed + sa_norm_column_start(a), out + sa_norm_column_start(a), den, a);
		if (b > 0)
			norm_column<RULE>(packed + sa_norm_column_start(b), out + sa_norm_column_start(b), den, b);
	}
}

std::atomic<double> g_last_normalize_seconds{ 0.0 };

hipError_t launch_denominators(sa_ctx *ctx, int32_t source, int32_t *d_den, hipStream_t s)
{
	if (source == SA_NORM_LENGTH) {
		const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)ctx->num + 255) / 256, 1024);
		hipLaunchKernelGGL(sa_k_lengths, dim3(blocks), dim3(256), 0, s, (const sa_meta *)ctx->d_meta, ctx->num, d_den);
		return hipGetLastError();
	}
	SelfArgs a{};
	a.st.codes = ctx->d_codes;
	a.st.meta = ctx->d_meta;
	a.st.num = ctx->num;
	a.sub = ctx->d_sub;
	a.gap_pen = ctx->sc.gap_pen;
	a.gap_opn = ctx->sc.gap_opn;
	a.gap_ext = ctx->sc.gap_ext;
	a.den = d_den;
	a.scratch = ctx->d_scratch;
	a.scratch_stride = ctx->scratch_stride;
	/* four waves per workgroup, a wave's scratch line per resident wave: never more workgroups than the context sized it for */
	const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->generic_blocks, ((int64_t)ctx->num + 3) / 4));
	switch (ctx->sc.method) {
	case SA_METHOD_NW:
		hipLaunchKernelGGL(sa_k_self<SA_METHOD_NW>, dim3(blocks), dim3(256), 0, s, a);
		break;
	case SA_METHOD_GA:
		hipLaunchKernelGGL(sa_k_self<SA_METHOD_GA>, dim3(blocks), dim3(256), 0, s, a);
		break;
	case SA_METHOD_SW:
		hipLaunchKernelGGL(sa_k_self<SA_METHOD_SW>, dim3(blocks), dim3(256), 0, s, a);
		break;
	default:
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t launch_normalize(const int32_t *packed, const int32_t *den, int32_t num, int32_t rule, int32_t *out, hipStream_t s)
{
	int device = 0, cus = 0;
	if (hipError_t e = hipGetDevice(&device); e != hipSuccess)
		return e;
	if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device); e != hipSuccess)
		return e;
	const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(sa_norm_units(num), (int64_t)std::max(cus, 1) * NORM_WGS_PER_CU));
	switch (rule) {
	case SA_NORM_MIN:
		hipLaunchKernelGGL(sa_k_normalize<SA_NORM_RULE_MIN>, dim3(wgs), dim3(NORM_THREADS), 0, s, packed, den, num, out);
		break;
	case SA_NORM_MAX:
		hipLaunchKernelGGL(sa_k_normalize<SA_NORM_RULE_MAX>, dim3(wgs), dim3(NORM_THREADS), 0, s, packed, den, num, out);
		break;
	case SA_NORM_MEAN:
		hipLaunchKernelGGL(sa_k_normalize<SA_NORM_RULE_MEAN>, dim3(wgs), dim3(NORM_THREADS), 0, s, packed, den, num, out);
		break;
	default:
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

bool source_ok(const char *who, int32_t source)
{
	if (source == SA_NORM_SELF || source == SA_NORM_LENGTH)
		return true;
	sa_set_error("%s: source %d is neither SA_NORM_SELF (%d) nor SA_NORM_LENGTH (%d)", who, source, (int)SA_NORM_SELF, (int)SA_NORM_LENGTH);
	return false;
}

bool rule_ok(const char *who, int32_t rule)
{
	if (rule == SA_NORM_MIN || rule == SA_NORM_MAX || rule == SA_NORM_MEAN)
		return true;
	sa_set_error("%s: rule %d is none of SA_NORM_MIN (%d), SA_NORM_MAX (%d), SA_NORM_MEAN (%d)", who, rule, (int)SA_NORM_MIN, (int)SA_NORM_MAX,
		     (int)SA_NORM_MEAN);
	return false;
}

} // namespace

/* for sa_search_quantity.hip (sa_ctx.h) */
bool sa_norm_rule_check(const char *who, int32_t rule) { return rule_ok(who, rule); }
hipError_t sa_denominators_launch(sa_ctx *ctx, int32_t source, int32_t *d_den, hipStream_t s) { return launch_denominators(ctx, source, d_den, s); }

/* what every entry point refuses before anything is launched */
bool sa_norm_check(const char *who, const struct sa_norm *norm)
{
	if (!norm) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	return source_ok(who, norm->source) && rule_ok(who, norm->rule);
}

/* Denominators + sweep in place over a finished device matrix of ctx's store, in order on `s`, which is synchronised: what the
 * *_norm calls and sa_zjob_normalize share.  The current device is the matrix's.  norm->denominators, when not null, receives
 * d[0 .. N); the device time of the two kernels goes to sa_hip_last_normalize_seconds.  false + sa_set_error on failure, nothing
 * written to the host. */
bool sa_normalize_in_place(const char *who, sa_ctx *ctx, int32_t *d_packed, const struct sa_norm *norm, hipStream_t s)
{
	struct Tmp {
		int32_t *d = nullptr;
		hipEvent_t e[2] = { nullptr, nullptr };
		~Tmp()
		{
			(void)hipFree(d);
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
		}
	} t;
	if (!sa_norm_check(who, norm))
		return false;
	std::vector<int32_t> h_den(norm->denominators ? (size_t)ctx->num : 0);
	SA_HIP_CHECK(hipMalloc(&t.d, sizeof(int32_t) * (size_t)ctx->num), return false);
	for (hipEvent_t &ev : t.e)
		SA_HIP_CHECK(hipEventCreate(&ev), return false);
	SA_HIP_CHECK(hipEventRecord(t.e[0], s), return false);
	SA_HIP_CHECK(launch_denominators(ctx, norm->source, t.d, s), return false);
	if (ctx->num >= 2) {
		SA_HIP_CHECK(launch_normalize(d_packed, t.d, ctx->num, norm->rule, d_packed, s), return false);
	}
	SA_HIP_CHECK(hipEventRecord(t.e[1], s), return false);
	if (!h_den.empty()) {
		SA_HIP_CHECK(hipMemcpyAsync(h_den.data(), t.d, sizeof(int32_t) * h_den.size(), hipMemcpyDeviceToHost, s), return false);
	}
	SA_HIP_CHECK(hipStreamSynchronize(s), return false);
	float ms = 0.f;
	SA_HIP_CHECK(hipEventElapsedTime(&ms, t.e[0], t.e[1]), return false);
	g_last_normalize_seconds.store((double)ms * 1e-3);
	if (!h_den.empty())
		std::copy(h_den.begin(), h_den.end(), norm->denominators);
	return true;
}

extern "C" int32_t sa_norm_value(int32_t s, int32_t di, int32_t dj, int32_t rule)
{
	return sa_guard("sa_norm_value", (int32_t)INT32_MIN, [&]() -> int32_t {
		if (!rule_ok("sa_norm_value", rule))
			return INT32_MIN;
		return sa_norm_value_rule(s, di, dj, rule);
	});
}

extern "C" int sa_ctx_denominators(sa_ctx *ctx, int32_t source, int32_t *d_den, void *stream)
{
	return sa_guard("sa_ctx_denominators", 1, [&] {
		if (!ctx || !d_den) {
			sa_set_error("sa_ctx_denominators: null argument");
			return 1;
		}
		if ((uintptr_t)d_den % 4) {
			sa_set_error("sa_ctx_denominators: d_den wants 4-byte alignment");
			return 1;
		}
		if (!source_ok("sa_ctx_denominators", source))
			return 1;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_denominators(ctx, source, d_den, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" int sa_ctx_normalize(sa_ctx *ctx, const int32_t *d_packed, const int32_t *d_den, int32_t rule, int32_t *d_out, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_normalize"))
		return 1;
	return sa_guard("sa_ctx_normalize", 1, [&] {
		if (!ctx || !d_packed || !d_den || !d_out) {
			sa_set_error("sa_ctx_normalize: null argument");
			return 1;
		}
		if ((uintptr_t)d_packed % 4 || (uintptr_t)d_den % 4 || (uintptr_t)d_out % 4) {
			sa_set_error("sa_ctx_normalize: d_packed, d_den and d_out want 4-byte alignment");
			return 1;
		}
		if (!rule_ok("sa_ctx_normalize", rule))
			return 1;
		if (ctx->num < 2) {
			sa_set_error("sa_ctx_normalize: %d sequences have no pair", ctx->num);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_normalize(d_packed, d_den, ctx->num, rule, d_out, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" double sa_hip_last_normalize_seconds(void)
{
	return sa_guard("sa_hip_last_normalize_seconds", 0.0, [&] { return g_last_normalize_seconds.load(); });
}
