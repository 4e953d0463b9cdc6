/*
 * sa_edges.hip -- the score graph: every pair that scores at least a threshold, as the symmetric adjacency in CSR form,
 * built where the scores are (sa_ctx_edge_offsets, sa_ctx_edge_fill, sa_hip_edges, sa_zjob_edges).  No reference counterpart:
 * the reference delivers the whole matrix and leaves the thresholding to the host.
 *
 * Input is the device-resident packed triangle (pair i < j at j (j - 1) / 2 + i).  Three steps in stream order, no host
 * synchronisation between them:
 *   count   sa_k_edges<false>: the sweep of sa_k_neighbors (sa_neighbors.hip) -- a workgroup owns R = 16 rows and walks all N
 *           columns in blocks of R x 64, left of the diagonal read along c, right of it along r and turned in LDS, the block that
 *           holds the diagonal element by element.  A wave owns a row of the block, one candidate per lane; the degree grows by
 *           the population count of the ballot.  The degree of row r goes to offsets[r + 1].
 *   scan    sa_k_edge_scan: one workgroup turns the degrees into offsets in place (offsets[0] = 0, then the inclusive sums).
 *   fill    sa_k_edges<true>: the same sweep with a wave-uniform 64-bit cursor per row that starts at offsets[r].  Column blocks
 *           come in ascending order and lanes are ascending columns, so a passing lane's place is the cursor + the passing lanes
 *           below it (ballot + mbcnt): ascending c without a sort, without atomics, and the same bytes whatever the timing.
 * The next block's loads are in flight while the current one is scanned, as in sa_k_neighbors.
 */
#include <atomic>
#include <new>

#include "sa_ctx.h"
#include "sa_edges_core.h"

struct sa_edges {
	int32_t num = 0;
	int64_t count = 0;
	int64_t *offsets = nullptr; /* num + 1 */
	int32_t *index = nullptr;   /* count (one element when count == 0: never a null pointer for a valid result) */
	int32_t *score = nullptr;
	~sa_edges()
	{
		free(offsets);
		free(index);
		free(score);
	}
};

namespace {

constexpr int EG_THREADS = 256; /* four waves */
constexpr int R = 16;           /* rows of a workgroup; divides 64 (sa_neighbors.hip: why 16) */
constexpr int Q = R / 4;        /* rows per wave = elements of a block per thread */

/* Block (rows r0 .. r0 + R, columns c0 .. c0 + 64): which thread holds which element in its Q registers.
 * `along_r`: strictly right of the diagonal -- lanes run along the rows, where the packed index is contiguous. */
__device__ __forceinline__ int eg_row(bool along_r, int tid, int q) { return along_r ? tid % R : (tid >> 6) + 4 * q; }
__device__ __forceinline__ int eg_col(bool along_r, int tid, int q) { return along_r ? tid / R + (EG_THREADS / R) * q : tid & 63; }

/* passing lanes below this one */
__device__ __forceinline__ int eg_below(uint64_t pass)
{
	return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(pass >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pass, 0u));
}

/* FILL = false: offsets[r + 1] = degree of r (offsets is written).  FILL = true: offsets is read, index / score are written;
 * a row never writes at or beyond offsets[r + 1], whatever the caller handed in. */
template <bool FILL>
__global__ __launch_bounds__(EG_THREADS) void sa_k_edges(const int32_t *__restrict__ packed, int32_t num, int32_t min_score,
							  int64_t *__restrict__ offsets, int32_t *__restrict__ index,
							  int32_t *__restrict__ score)
{
	__shared__ int32_t turn[R][65];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t r0 = (int64_t)blockIdx.x * R;
	const int blocks = (num + 63) / 64, diag = (int)(r0 / 64); /* (R divides 64: exactly one column block holds the diagonal) */

	int64_t cursor[Q], end[Q]; /* row r0 + wave + 4 q (wave-uniform): count: the degree so far; fill: the next free place */
#pragma unroll
	for (int q = 0; q < Q; q++) {
		const int64_t r = r0 + wave + 4 * q;
		cursor[q] = FILL && r < num ? offsets[r] : 0;
		end[q] = FILL && r < num ? offsets[r + 1] : 0;
	}

	int32_t regs[Q];
	auto fetch = [&](int b) {
		const int64_t c0 = (int64_t)b * 64;
		const bool along_r = b > diag;
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const int64_t i = r0 + eg_row(along_r, tid, q), j = c0 + eg_col(along_r, tid, q);
			int32_t v = 0;
			if (i < num && j < num && i != j) {
				if (b < diag)
					v = packed[sa_edge_left_at(i, j)];
				else if (along_r)
					v = packed[sa_edge_right_at(i, j)];
				else
					v = packed[sa_nb_packed_at(i, j)];
			}
			regs[q] = v;
		}
	};

	fetch(0);
	for (int b = 0; b < blocks; b++) {
		const bool along_r = b > diag;
#pragma unroll
		for (int q = 0; q < Q; q++)
			turn[eg_row(along_r, tid, q)][eg_col(along_r, tid, q)] = regs[q];
		__syncthreads();
		if (b + 1 < blocks)
			fetch(b + 1); /* in flight while this block is scanned */
		const int64_t c = (int64_t)b * 64 + lane;
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const int y = wave + 4 * q;
			const int64_t r = r0 + y;
			if (r >= num) /* (wave-uniform) */
				continue;
			const int32_t v = turn[y][lane];
			const bool mine = c < num && c != r && sa_edge_pass(v, min_score);
			const uint64_t pass = __ballot(mine);
			if (FILL) {
				const int64_t at = cursor[q] + eg_below(pass);
				if (mine && at < end[q]) {
					index[at] = (int32_t)c;
					score[at] = v;
				}
			}
			cursor[q] += __popcll(pass);
		}
		__syncthreads();
	}
	if (!FILL) {
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const int64_t r = r0 + wave + 4 * q;
			if (r < num && lane == 0)
				offsets[r + 1] = cursor[q];
		}
	}
}

/* One workgroup: offsets[1 .. num] hold the degrees; afterwards offsets[0] = 0 and offsets[r + 1] = the sum of the degrees of
 * rows 0 .. r.  In place: every thread reads its element before the tile's barrier and writes it after. */
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void sa_k_edge_scan(int64_t *__restrict__ offsets, int32_t num)
{
	__shared__ int64_t wave_sum[SCAN_THREADS / 64];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int64_t carry = 0; /* the sum of every tile before this one (the same in every thread) */
	if (tid == 0)
		offsets[0] = 0;
	for (int64_t base = 0; base < num; base += SCAN_THREADS) {
		const int64_t r = base + tid;
		int64_t v = r < num ? offsets[r + 1] : 0;
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
		if (r < num)
			offsets[r + 1] = carry + before + v;
		carry += tile;
		__syncthreads();
	}
}

std::atomic<double> g_last_edges_seconds{ 0.0 };

hipError_t launch_offsets(const int32_t *packed, int32_t num, int32_t min_score, int64_t *offsets, hipStream_t s)
{
	hipLaunchKernelGGL(sa_k_edges<false>, dim3((unsigned)((num + R - 1) / R)), dim3(EG_THREADS), 0, s, packed, num, min_score, offsets,
			   (int32_t *)nullptr, (int32_t *)nullptr);
	if (hipError_t e = hipGetLastError(); e != hipSuccess)
		return e;
	hipLaunchKernelGGL(sa_k_edge_scan, dim3(1), dim3(SCAN_THREADS), 0, s, offsets, num);
	return hipGetLastError();
}

hipError_t launch_fill(const int32_t *packed, int32_t num, int32_t min_score, const int64_t *offsets, int32_t *index, int32_t *score,
		       hipStream_t s)
{
	hipLaunchKernelGGL(sa_k_edges<true>, dim3((unsigned)((num + R - 1) / R)), dim3(EG_THREADS), 0, s, packed, num, min_score,
			   const_cast<int64_t *>(offsets), index, score);
	return hipGetLastError();
}

} // namespace

/* The graph of a finished device matrix into HOST arrays, in order on `s`: what sa_hip_edges and sa_zjob_edges share.  The
 * current device is the matrix's.  After the count the host reads E (8 bytes) and allocates exactly 8 E bytes of device
 * memory.  Leaves the device time of count + scan + fill for sa_hip_last_edges_seconds.  nullptr + sa_set_error on failure. */
sa_edges *sa_edges_to_host(const char *who, const int32_t *d_packed, int32_t num, int32_t min_score, hipStream_t s)
{
	struct Tmp {
		int64_t *d_offsets = nullptr;
		int32_t *d_out = nullptr;
		hipEvent_t e[4] = { nullptr, nullptr, nullptr, nullptr };
		sa_edges *res = nullptr;
		~Tmp()
		{
			(void)hipFree(d_offsets);
			(void)hipFree(d_out);
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
			delete res;
		}
	} t;
	if (num < 1) {
		sa_set_error("%s: %d sequences", who, num);
		return nullptr;
	}
	t.res = new sa_edges;
	t.res->num = num;
	t.res->offsets = (int64_t *)malloc(sizeof(int64_t) * ((size_t)num + 1));
	if (!t.res->offsets) {
		sa_set_error("%s: out of host memory for the offsets of %d sequences", who, num);
		return nullptr;
	}
	SA_HIP_CHECK(hipMalloc(&t.d_offsets, sizeof(int64_t) * ((size_t)num + 1)), return nullptr);
	for (hipEvent_t &ev : t.e)
		SA_HIP_CHECK(hipEventCreate(&ev), return nullptr);
	SA_HIP_CHECK(hipEventRecord(t.e[0], s), return nullptr);
	SA_HIP_CHECK(launch_offsets(d_packed, num, min_score, t.d_offsets, s), return nullptr);
	SA_HIP_CHECK(hipEventRecord(t.e[1], s), return nullptr);
	SA_HIP_CHECK(hipMemcpyAsync(t.res->offsets, t.d_offsets, sizeof(int64_t) * ((size_t)num + 1), hipMemcpyDeviceToHost, s), return nullptr);
	SA_HIP_CHECK(hipStreamSynchronize(s), return nullptr);
	const int64_t count = t.res->offsets[num];
	t.res->count = count;
	const size_t elems = (size_t)count, room = elems ? elems : 1;
	t.res->index = (int32_t *)malloc(sizeof(int32_t) * room);
	t.res->score = (int32_t *)malloc(sizeof(int32_t) * room);
	if (!t.res->index || !t.res->score) {
		sa_set_error("%s: the %lld edges of %d sequences (%.2f GiB) do not fit the host's memory", who, (long long)count, num,
			     (double)elems * 8.0 / (double)(1 << 30));
		return nullptr;
	}
	float ms_count = 0.f, ms_fill = 0.f;
	if (elems) {
		if (hipMalloc(&t.d_out, 2 * elems * sizeof(int32_t)) != hipSuccess) {
			(void)hipGetLastError();
			t.d_out = nullptr;
			sa_set_error("%s: the %lld edges of %d sequences (%.2f GiB) do not fit the device's memory", who, (long long)count, num,
				     (double)elems * 8.0 / (double)(1 << 30));
			return nullptr;
		}
		SA_HIP_CHECK(hipEventRecord(t.e[2], s), return nullptr);
		SA_HIP_CHECK(launch_fill(d_packed, num, min_score, t.d_offsets, t.d_out, t.d_out + elems, s), return nullptr);
		SA_HIP_CHECK(hipEventRecord(t.e[3], s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(t.res->index, t.d_out, elems * sizeof(int32_t), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(t.res->score, t.d_out + elems, elems * sizeof(int32_t), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipStreamSynchronize(s), return nullptr);
		SA_HIP_CHECK(hipEventElapsedTime(&ms_fill, t.e[2], t.e[3]), return nullptr);
	}
	SA_HIP_CHECK(hipEventElapsedTime(&ms_count, t.e[0], t.e[1]), return nullptr);
	g_last_edges_seconds.store(((double)ms_count + (double)ms_fill) * 1e-3);
	sa_edges *res = t.res;
	t.res = nullptr;
	return res;
}

extern "C" int sa_ctx_edge_offsets(sa_ctx *ctx, const int32_t *d_packed, int32_t min_score, int64_t *d_offsets, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_edge_offsets"))
		return 1;
	return sa_guard("sa_ctx_edge_offsets", 1, [&] {
		if (!ctx || !d_packed || !d_offsets) {
			sa_set_error("sa_ctx_edge_offsets: null argument");
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_offsets(d_packed, ctx->num, min_score, d_offsets, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" int sa_ctx_edge_fill(sa_ctx *ctx, const int32_t *d_packed, int32_t min_score, const int64_t *d_offsets, int32_t *d_index,
				int32_t *d_score, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_edge_fill"))
		return 1;
	return sa_guard("sa_ctx_edge_fill", 1, [&] {
		if (!ctx || !d_packed || !d_offsets || !d_index || !d_score) {
			sa_set_error("sa_ctx_edge_fill: null argument");
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_fill(d_packed, ctx->num, min_score, d_offsets, d_index, d_score, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" const int64_t *sa_edges_offsets(const sa_edges *e, int32_t *num)
{
	return sa_guard("sa_edges_offsets", (const int64_t *)nullptr, [&] {
		if (num)
			*num = e ? e->num : 0;
		return e ? (const int64_t *)e->offsets : nullptr;
	});
}

extern "C" const int32_t *sa_edges_index(const sa_edges *e, int64_t *count)
{
	return sa_guard("sa_edges_index", (const int32_t *)nullptr, [&] {
		if (count)
			*count = e ? e->count : 0;
		return e ? (const int32_t *)e->index : nullptr;
	});
}

extern "C" const int32_t *sa_edges_score(const sa_edges *e)
{
	return sa_guard("sa_edges_score", (const int32_t *)nullptr, [&] { return e ? (const int32_t *)e->score : nullptr; });
}

extern "C" void sa_edges_destroy(sa_edges *e)
{
	sa_guard_void("sa_edges_destroy", [&] { delete e; });
}

extern "C" double sa_hip_last_edges_seconds(void)
{
	return sa_guard("sa_hip_last_edges_seconds", 0.0, [&] { return g_last_edges_seconds.load(); });
}
