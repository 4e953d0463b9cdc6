/*
 * sa_select.hip -- exact order statistics of the score distribution: the k-th smallest entry of the device-resident packed
 * triangle and the number of entries below it, for up to SA_HIP_SELECT_MAX ranks at once (sa_ctx_select, sa_hip_select,
 * sa_zjob_select, and the cut of sa_hip_edges_at_rank / sa_hip_linkage_with_ranks).  No reference counterpart: the reference
 * delivers the whole matrix and leaves its distribution to the host.
 *
 * A radix select over the keys of sa_select_core.h, most significant byte first, nine kernels in stream order without the host:
 *   start   sa_k_sel_start: the ranks (kernel arguments) into the state, the table zeroed -- everything the rounds read, so the
 *           contents of the scratch memory never matter.
 *   count   sa_k_sel_count, once per round: a persistent grid (SEL_WGS_PER_CU workgroups per CU) strides over the P entries with
 *           16-byte loads over the aligned body; the up to three entries before it and after it go element by element to the
 *           first wave of workgroup 0, so d_packed needs no more than its natural 4-byte alignment.  An entry that shares a
 *           group's prefix (at most 16, wave-uniform, held in scalar registers) counts in the workgroup's LDS table
 *           uint32[groups][256] by its byte of the round; the others are dropped.  At the end the workgroup adds its non-zero
 *           bins to the global 64-bit table with vector atomics.
 *   narrow  sa_k_sel_narrow, once per round, one workgroup: takes the table into LDS and zeroes it for the next round; a thread
 *           per rank walks its group's 256 bins (sa_sel_narrow); thread 0 rebuilds the groups (sa_sel_regroup).  After the last
 *           round the threads write value and below.
 *
 * Real scores share their upper bytes: in rounds 0 .. 2 the 64 lanes of a wave hit one or two bins, and an LDS atomic per lane
 * would serialise.  So a wave aggregates first: the first pending lane's bin is broadcast, the lanes that share it are balloted,
 * that one lane adds the population count; after SEL_PEELS such peels the lanes still pending add 1 each (round 3, and every
 * round of uniformly random data, spread over all bins).  Counts are sums of integers: both ways, and any order of waves and
 * workgroups, give the same table, so the result is the same bytes run after run.
 *
 * 32-bit LDS counts: a workgroup sees at most P / gridDim + 1024 + 6 entries, and the launch keeps gridDim >= P / 2^31, so no
 * LDS bin can pass 2^31 + 1030.  Everything global -- the table, remain, below, the indices -- is 64-bit.
 */
#include <algorithm>
#include <atomic>

#include "sa_ctx.h"
#include "sa_select_core.h"

namespace {

constexpr int SEL_THREADS = 256;  /* four waves */
constexpr int SEL_WGS_PER_CU = 4; /* 16 KB of LDS each */
constexpr int SEL_UNROLL = 4;     /* 16-byte loads in flight per thread */
constexpr int SEL_PEELS = 2;      /* wave-aggregated adds before the per-lane ones */

struct SelRanks {
	int64_t rank[SA_SEL_MAX];
};

/* one workgroup: everything the rounds read */
__global__ __launch_bounds__(SEL_THREADS) void sa_k_sel_start(sa_sel_state *__restrict__ st, uint64_t *__restrict__ table, SelRanks ranks,
							       int32_t m)
{
	const int tid = threadIdx.x;
	if (tid < SA_SEL_MAX) {
		sa_sel_start(st, tid, tid < m ? ranks.rank[tid] : 0);
		st->group_prefix[tid] = 0;
	}
	for (int b = tid; b < m * SA_SEL_BINS; b += SEL_THREADS)
		table[b] = 0;
}

/* one entry per lane (slot < 0: none) into the workgroup's table; every lane of the wave calls this */
__device__ __forceinline__ void sel_add(uint32_t *local, int slot, int lane)
{
	bool pending = slot >= 0;
#pragma unroll
	for (int peel = 0; peel < SEL_PEELS; peel++) {
		const uint64_t live = __ballot(pending);
		if (!live) /* (wave-uniform) */
			return;
		const int lead = __ffsll((unsigned long long)live) - 1;
		const int s = __builtin_amdgcn_readlane(slot, lead);
		const bool same = pending && slot == s;
		const uint64_t sharing = __ballot(same);
		if (lane == lead)
			atomicAdd(&local[s], (uint32_t)__popcll(sharing));
		pending = pending && !same;
	}
	if (pending)
		atomicAdd(&local[slot], 1u);
}

/* packed[0 .. head) and packed[head + 4 vecs .. pairs) are the unaligned ends (at most 3 entries each), packed + head is
 * 16-byte aligned */
__global__ __launch_bounds__(SEL_THREADS) void sa_k_sel_count(const int32_t *__restrict__ packed, int64_t pairs, int32_t head, int64_t vecs,
							       const sa_sel_state *__restrict__ st, uint64_t *__restrict__ table, int32_t round)
{
	__shared__ uint32_t local[SA_SEL_MAX * SA_SEL_BINS];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int32_t groups = min(max(st->groups, 1), SA_SEL_MAX);
	uint32_t upper[SA_SEL_MAX]; /* the groups' upper bits (wave-uniform, indexed by unrolled loops only); no key has those of an unused one */
#pragma unroll
	for (int g = 0; g < SA_SEL_MAX; g++)
		upper[g] = g < groups ? sa_sel_upper(st->group_prefix[g], round) : SA_SEL_NO_UPPER;
	for (int b = tid; b < groups * SA_SEL_BINS; b += SEL_THREADS)
		local[b] = 0;
	__syncthreads();

	auto slot_of = [&](int32_t score) {
		const uint32_t key = sa_sel_key(score);
		const uint32_t mine = sa_sel_upper(key, round);
		int found = -1;
#pragma unroll
		for (int g = 0; g < SA_SEL_MAX; g++) {
			if (g % 4 == 0 && g >= groups) /* (wave-uniform) */
				break;
			found = mine == upper[g] ? g : found;
		}
		return found < 0 ? -1 : found * SA_SEL_BINS + (int)sa_sel_byte(key, round);
	};

	const int4 *__restrict__ body = reinterpret_cast<const int4 *>(packed + head);
	const int64_t stride = (int64_t)gridDim.x * SEL_THREADS;
	for (int64_t base = (int64_t)blockIdx.x * SEL_THREADS; base < vecs; base += stride * SEL_UNROLL) { /* (uniform in the workgroup) */
		int4 v[SEL_UNROLL];
		bool have[SEL_UNROLL];
#pragma unroll
		for (int u = 0; u < SEL_UNROLL; u++) {
			const int64_t i = base + (int64_t)u * stride + tid;
			have[u] = i < vecs;
			v[u] = have[u] ? body[i] : make_int4(0, 0, 0, 0);
		}
#pragma unroll
		for (int u = 0; u < SEL_UNROLL; u++) {
			sel_add(local, have[u] ? slot_of(v[u].x) : -1, lane);
			sel_add(local, have[u] ? slot_of(v[u].y) : -1, lane);
			sel_add(local, have[u] ? slot_of(v[u].z) : -1, lane);
			sel_add(local, have[u] ? slot_of(v[u].w) : -1, lane);
		}
	}
	if (blockIdx.x == 0 && wave == 0) { /* the ends: fewer than 8 entries */
		const int64_t tail_at = (int64_t)head + 4 * vecs;
		const int64_t at = lane < head ? (int64_t)lane : tail_at + (lane - head);
		sel_add(local, at < pairs ? slot_of(packed[at]) : -1, lane);
	}
	__syncthreads();
	for (int b = tid; b < groups * SA_SEL_BINS; b += SEL_THREADS) {
		const uint32_t n = local[b];
		if (n)
			atomicAdd(reinterpret_cast<unsigned long long *>(&table[b]), (unsigned long long)n);
	}
}

/* one workgroup; value / below are written after the last round only */
__global__ __launch_bounds__(SEL_THREADS) void sa_k_sel_narrow(sa_sel_state *st, uint64_t *table, int32_t m,
								int32_t round, int32_t *__restrict__ value, int64_t *__restrict__ below)
{
	__shared__ uint64_t bins[SA_SEL_MAX * SA_SEL_BINS];
	const int tid = threadIdx.x;
	for (int b = tid; b < m * SA_SEL_BINS; b += SEL_THREADS) {
		bins[b] = table[b];
		table[b] = 0;
	}
	__syncthreads();
	if (tid < m) {
		sa_sel_narrow(st, bins, tid, round);
		if (round == SA_SEL_ROUNDS - 1) {
			value[tid] = sa_sel_score(st->prefix[tid]);
			below[tid] = st->below[tid];
		}
	}
	__syncthreads();
	if (tid == 0 && round < SA_SEL_ROUNDS - 1)
		sa_sel_regroup(st, m);
}

std::atomic<double> g_last_select_seconds{ 0.0 };

/* start + 4 x (count, narrow) on `s`; the current device is the matrix's; arguments checked by the caller */
hipError_t launch_select(const int32_t *packed, int64_t pairs, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below, void *scratch,
			 hipStream_t s)
{
	int device = 0, cus = 0;
	if (hipError_t e = hipGetDevice(&device); e != hipSuccess)
		return e;
	if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device); e != hipSuccess)
		return e;
	sa_sel_state *st = (sa_sel_state *)scratch;
	uint64_t *table = (uint64_t *)((char *)scratch + sa_sel_table_offset());
	SelRanks args{};
	for (int32_t t = 0; t < m; t++)
		args.rank[t] = ranks[t];
	const int64_t head = std::min<int64_t>(pairs, (int64_t)(((16 - ((uintptr_t)packed & 15)) & 15) / 4));
	const int64_t vecs = (pairs - head) / 4;
	int64_t wgs = std::min<int64_t>((int64_t)std::max(cus, 1) * SEL_WGS_PER_CU, (vecs + SEL_THREADS - 1) / SEL_THREADS);
	wgs = std::max<int64_t>(std::max<int64_t>(wgs, 1), (pairs >> 31) + 1); /* (the bound of the 32-bit LDS counts) */
	hipLaunchKernelGGL(sa_k_sel_start, dim3(1), dim3(SEL_THREADS), 0, s, st, table, args, m);
	if (hipError_t e = hipGetLastError(); e != hipSuccess)
		return e;
	for (int round = 0; round < SA_SEL_ROUNDS; round++) {
		hipLaunchKernelGGL(sa_k_sel_count, dim3((unsigned)wgs), dim3(SEL_THREADS), 0, s, packed, pairs, (int32_t)head, vecs,
				   (const sa_sel_state *)st, table, (int32_t)round);
		if (hipError_t e = hipGetLastError(); e != hipSuccess)
			return e;
		hipLaunchKernelGGL(sa_k_sel_narrow, dim3(1), dim3(SEL_THREADS), 0, s, st, table, m, (int32_t)round, value, below);
		if (hipError_t e = hipGetLastError(); e != hipSuccess)
			return e;
	}
	return hipSuccess;
}

} // namespace

/* what every entry point refuses before anything is launched: m, N and the ranks (a host array) */
bool sa_select_check(const char *who, int32_t num, const int64_t *ranks, int32_t m)
{
	if (!ranks) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (m < 1 || m > SA_SEL_MAX) {
		sa_set_error("%s: %d ranks (1 .. %d in one call)", who, m, SA_SEL_MAX);
		return false;
	}
	if (num < 2) {
		sa_set_error("%s: %d sequences have no pair", who, num);
		return false;
	}
	const int64_t pairs = (int64_t)num * (num - 1) / 2;
	for (int32_t t = 0; t < m; t++)
		if (ranks[t] < 0 || ranks[t] >= pairs) {
			sa_set_error("%s: rank %lld (number %d) is outside [0, %lld), the pairs of %d sequences", who, (long long)ranks[t], t,
				     (long long)pairs, num);
			return false;
		}
	return true;
}

/* The order statistics of a finished device matrix into HOST arrays, in order on `s`, which is synchronised: what sa_hip_select,
 * sa_zjob_select and the *_at_rank / *_with_ranks calls share.  The current device is the matrix's.  Leaves the device time of
 * the nine kernels for sa_hip_last_select_seconds.  false + sa_set_error on failure, nothing written. */
bool sa_select_to_host(const char *who, const int32_t *d_packed, int32_t num, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below,
		       hipStream_t s)
{
	struct Tmp {
		char *d = nullptr;
		hipEvent_t e[2] = { nullptr, nullptr };
		~Tmp()
		{
			(void)hipFree(d);
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
		}
	} t;
	if (!value || !below) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (!sa_select_check(who, num, ranks, m))
		return false;
	const int64_t pairs = (int64_t)num * (num - 1) / 2;
	const size_t scratch = sa_sel_scratch_bytes(m), below_bytes = sizeof(int64_t) * (size_t)m, value_bytes = sizeof(int32_t) * (size_t)m;
	SA_HIP_CHECK(hipMalloc(&t.d, below_bytes + scratch + value_bytes), return false); /* (8-byte things first) */
	int64_t *d_below = (int64_t *)t.d;
	void *d_scratch = t.d + below_bytes;
	int32_t *d_value = (int32_t *)(t.d + below_bytes + scratch);
	for (hipEvent_t &ev : t.e)
		SA_HIP_CHECK(hipEventCreate(&ev), return false);
	int32_t h_value[SA_SEL_MAX];
	int64_t h_below[SA_SEL_MAX];
	SA_HIP_CHECK(hipEventRecord(t.e[0], s), return false);
	SA_HIP_CHECK(launch_select(d_packed, pairs, ranks, m, d_value, d_below, d_scratch, s), return false);
	SA_HIP_CHECK(hipEventRecord(t.e[1], s), return false);
	SA_HIP_CHECK(hipMemcpyAsync(h_value, d_value, value_bytes, hipMemcpyDeviceToHost, s), return false);
	SA_HIP_CHECK(hipMemcpyAsync(h_below, d_below, below_bytes, hipMemcpyDeviceToHost, s), return false);
	SA_HIP_CHECK(hipStreamSynchronize(s), return false);
	float ms = 0.f;
	SA_HIP_CHECK(hipEventElapsedTime(&ms, t.e[0], t.e[1]), return false);
	g_last_select_seconds.store((double)ms * 1e-3);
	for (int32_t k = 0; k < m; k++) {
		value[k] = h_value[k];
		below[k] = h_below[k];
	}
	return true;
}

extern "C" size_t sa_select_scratch_bytes(int32_t m) { return sa_sel_scratch_bytes(m); }

extern "C" int64_t sa_score_rank(int64_t pairs, double q) { return sa_sel_rank(pairs, q); }

extern "C" int sa_ctx_select(sa_ctx *ctx, const int32_t *d_packed, const int64_t *ranks, int32_t m, int32_t *d_value, int64_t *d_below,
			     void *d_scratch, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_select"))
		return 1;
	return sa_guard("sa_ctx_select", 1, [&] {
		if (!ctx || !d_packed || !ranks || !d_value || !d_below || !d_scratch) {
			sa_set_error("sa_ctx_select: null argument");
			return 1;
		}
		if ((uintptr_t)d_scratch % 8 || (uintptr_t)d_below % 8 || (uintptr_t)d_value % 4 || (uintptr_t)d_packed % 4) {
			sa_set_error("sa_ctx_select: the scratch memory and d_below want 8-byte alignment, d_packed and d_value 4-byte");
			return 1;
		}
		if (!sa_select_check("sa_ctx_select", ctx->num, ranks, m))
			return 1;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_select(d_packed, (int64_t)ctx->num * (ctx->num - 1) / 2, ranks, m, d_value, d_below, d_scratch, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" double sa_hip_last_select_seconds(void)
{
	return sa_guard("sa_hip_last_select_seconds", 0.0, [&] { return g_last_select_seconds.load(); });
}
