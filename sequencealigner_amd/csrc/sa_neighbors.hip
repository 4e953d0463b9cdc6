/*
 * sa_neighbors.hip -- the k best partners of every sequence, selected where the scores are (sa_ctx_neighbors,
 * sa_hip_neighbors, sa_zjob_neighbors).  No reference counterpart: the reference delivers the whole matrix and leaves
 * clustering / nearest-hit lookup to a sort of every row on the host.
 *
 * Input is the device-resident packed triangle (pair i < j at j (j - 1) / 2 + i).  Row r of the symmetric matrix is two
 * pieces: for c < r a run of the packed index, for c > r one element per column -- but consecutive rows of one column
 * are contiguous.  So a workgroup owns a block of R = 16 rows and sweeps all N columns in blocks of R x 64: left of the diagonal
 * the block is read along c, right of it along r and turned in LDS (what sa_k_tiles_raw does, sa_deflate.hip), so both
 * halves move whole runs; the one block that holds the diagonal is read element by element.  Because a workgroup owns its
 * rows outright there is no partial-list merge and no scratch memory.
 *
 * A wave scans one row of the block at a time, one candidate per lane.  The row's list lives one entry per lane, in
 * descending key order (sa_neighbors_core.h: the key is the contract -- score descending, index ascending); that is what
 * k <= 64 buys on wave64.  A candidate is compared with the k-th entry first: after the first blocks a ballot finds almost
 * none that pass (about k (1 + ln(N / k)) insertions per row), and an insertion is a ballot + population count for the
 * position and a one-lane DPP shift.  The next block's loads are in flight while the current one is scanned.
 *
 * Why 16 rows: the kernel is bound by latency, not by bytes -- a lower block puts more workgroups on the device (N / R of them,
 * 42 VGPRs each) and that outweighs the shorter runs right of the diagonal (R x 4 bytes).  Measured with R = 16 / 32 / 64 at
 * k = 64: 0.48 / 0.76 / 1.25 ms for 10 000 rows, 2.9 / 3.3 / 4.4 ms for 40 000.
 */
#include <atomic>

#include "sa_ctx.h"
#include "sa_neighbors_core.h"

namespace {

constexpr int NB_THREADS = 256; /* four waves */

__device__ __forceinline__ uint64_t nb_readlane(uint64_t v, int lane) /* lane: wave-uniform */
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
	return ((uint64_t)hi << 32) | lo;
}

/* lane l receives lane l - 1's value (wave_shr:1, all 64 lanes); lane 0 keeps its own */
__device__ __forceinline__ uint64_t nb_shift_down(uint64_t v)
{
	const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
	const uint32_t slo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
	const uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
	return ((uint64_t)shi << 32) | slo;
}

constexpr int R = 16;    /* rows of a workgroup; divides 64 */
constexpr int Q = R / 4; /* rows per wave = elements of a block per thread */

/* Block (rows r0 .. r0 + R, columns c0 .. c0 + 64): which thread holds which element in its Q registers.
 * `along_r`: strictly right of the diagonal -- lanes run along the rows, where the packed index is contiguous. */
__device__ __forceinline__ int nb_row(bool along_r, int tid, int q) { return along_r ? tid % R : (tid >> 6) + 4 * q; }
__device__ __forceinline__ int nb_col(bool along_r, int tid, int q) { return along_r ? tid / R + (NB_THREADS / R) * q : tid & 63; }

__global__ __launch_bounds__(NB_THREADS) void sa_k_neighbors(const int32_t *__restrict__ packed, int32_t num, int32_t k,
							     int32_t *__restrict__ index, int32_t *__restrict__ score)
{
	__shared__ int32_t turn[R][65];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t r0 = (int64_t)blockIdx.x * R;
	const int blocks = (num + 63) / 64, diag = (int)(r0 / 64); /* (R divides 64: exactly one column block holds the diagonal) */

	uint64_t list[Q]; /* row r0 + wave + 4 q: this lane's entry */
#pragma unroll
	for (int q = 0; q < Q; q++)
		list[q] = SA_NB_EMPTY;

	int32_t regs[Q];
	auto fetch = [&](int b) {
		const int64_t c0 = (int64_t)b * 64;
		const bool along_r = b > diag;
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const int64_t i = r0 + nb_row(along_r, tid, q), j = c0 + nb_col(along_r, tid, q);
			int32_t v = 0;
			if (i < num && j < num && i != j) {
				if (b < diag)
					v = packed[i * (i - 1) / 2 + j];
				else if (along_r)
					v = packed[j * (j - 1) / 2 + i];
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
			turn[nb_row(along_r, tid, q)][nb_col(along_r, tid, q)] = regs[q];
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
			const uint64_t x = c < num && c != r ? sa_nb_key(turn[y][lane], (int32_t)c) : SA_NB_EMPTY;
			uint64_t mine = list[q];
			uint64_t kth = nb_readlane(mine, k - 1);
			uint64_t pass = __ballot(x > kth);
			while (pass) {
				const int from = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(pass));
				pass &= pass - 1;
				const uint64_t cand = nb_readlane(x, from);
				if (cand > kth) { /* (the k-th entry has moved since the ballot) */
					const int pos = __popcll(__ballot(mine > cand));
					const uint64_t above = nb_shift_down(mine);
					mine = lane < pos ? mine : lane == pos ? cand : above;
					kth = nb_readlane(mine, k - 1);
				}
			}
			list[q] = mine;
		}
		__syncthreads();
	}
#pragma unroll
	for (int q = 0; q < Q; q++) {
		const int64_t r = r0 + wave + 4 * q;
		if (r < num && lane < k) {
			index[r * k + lane] = sa_nb_key_index(list[q]);
			score[r * k + lane] = sa_nb_key_score(list[q]);
		}
	}
}

std::atomic<double> g_last_neighbors_seconds{ 0.0 };

} // namespace

bool sa_neighbors_check(const char *who, int64_t num, int32_t k)
{
	if (k < 1 || k > SA_HIP_NEIGHBORS_MAX || (int64_t)k > num - 1) {
		sa_set_error("%s: k = %d neighbours of %lld sequences: k must be in [1, min(N - 1, %d)]", who, k, (long long)num, SA_HIP_NEIGHBORS_MAX);
		return false;
	}
	return true;
}

hipError_t sa_launch_neighbors(const int32_t *packed, int32_t num, int32_t k, int32_t *index, int32_t *score, hipStream_t s)
{
	hipLaunchKernelGGL(sa_k_neighbors, dim3((unsigned)((num + R - 1) / R)), dim3(NB_THREADS), 0, s, packed, num, k, index, score);
	return hipGetLastError();
}

/* the selection over a finished device matrix into HOST arrays, in order on `s`: what sa_hip_neighbors and sa_zjob_neighbors
 * share.  The current device is the matrix's.  Leaves the kernel's device time for sa_hip_last_neighbors_seconds. */
bool sa_neighbors_to_host(const int32_t *d_packed, int32_t num, int32_t k, int32_t *index, int32_t *score, hipStream_t s)
{
	struct Tmp {
		int32_t *d_out = nullptr;
		hipEvent_t e0 = nullptr, e1 = nullptr;
		~Tmp()
		{
			(void)hipFree(d_out);
			if (e0)
				(void)hipEventDestroy(e0);
			if (e1)
				(void)hipEventDestroy(e1);
		}
	} t;
	const size_t elems = (size_t)num * (size_t)k;
	SA_HIP_CHECK(hipMalloc(&t.d_out, 2 * elems * sizeof(int32_t)), return false);
	SA_HIP_CHECK(hipEventCreate(&t.e0), return false);
	SA_HIP_CHECK(hipEventCreate(&t.e1), return false);
	SA_HIP_CHECK(hipEventRecord(t.e0, s), return false);
	SA_HIP_CHECK(sa_launch_neighbors(d_packed, num, k, t.d_out, t.d_out + elems, s), return false);
	SA_HIP_CHECK(hipEventRecord(t.e1, s), return false);
	SA_HIP_CHECK(hipMemcpyAsync(index, t.d_out, elems * sizeof(int32_t), hipMemcpyDeviceToHost, s), return false);
	SA_HIP_CHECK(hipMemcpyAsync(score, t.d_out + elems, elems * sizeof(int32_t), hipMemcpyDeviceToHost, s), return false);
	SA_HIP_CHECK(hipStreamSynchronize(s), return false);
	float ms = 0.f;
	SA_HIP_CHECK(hipEventElapsedTime(&ms, t.e0, t.e1), return false);
	g_last_neighbors_seconds.store((double)ms * 1e-3);
	return true;
}

extern "C" int sa_ctx_neighbors(sa_ctx *ctx, const int32_t *d_packed, int32_t k, int32_t *d_index, int32_t *d_score, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_neighbors"))
		return 1;
	return sa_guard("sa_ctx_neighbors", 1, [&] {
		if (!ctx || !d_packed || !d_index || !d_score) {
			sa_set_error("sa_ctx_neighbors: null argument");
			return 1;
		}
		if (!sa_neighbors_check("sa_ctx_neighbors", ctx->num, k))
			return 1;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(sa_launch_neighbors(d_packed, ctx->num, k, d_index, d_score, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" double sa_hip_last_neighbors_seconds(void)
{
	return sa_guard("sa_hip_last_neighbors_seconds", 0.0, [&] { return g_last_neighbors_seconds.load(); });
}
