/*
 * sa_generic.hip -- the "pair per wavefront" score kernel (gfx950, wave64) and the small kernels that arrange scores
 * (expand, widen, place).
 *
 * sa_k_pair_per_wave<METHOD> is the always-applicable path: one (i,j) pair per wavefront through the anti-diagonal s32
 * sweep of sa_wave_sweep.inc (rows: seq i, columns: seq j).
 *
 * It is the fallback of the systolic streaming kernels (sa_systolic.hip), which need bounded scores and len <= their
 * column budget; this one does not.
 */
#include <algorithm>
#include "sa_wave_sweep.h"

namespace {

template <int METHOD>
__global__ __launch_bounds__(256) void sa_k_pair_per_wave(SaGenericArgs A)
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

	for (int64_t q = wave; q < A.count; q += nwaves) {
		int32_t i, j;
		unpack_pair(A.start + q, i, j);
		const int32_t m = A.st.meta[i].len, offi = A.st.meta[i].off; /* rows: seq i */
		const int32_t n = A.st.meta[j].len, offj = A.st.meta[j].off; /* cols: seq j */
		const uint8_t *ci = A.st.codes + offi;
		const uint8_t *cj = A.st.codes + offj;
#include "sa_wave_sweep.inc"
		const int32_t score = METHOD == SA_METHOD_SW ? wave_max(best) : mn;
		if (lane == 0) {
			if (A.out16)
				reinterpret_cast<int16_t *>(A.out)[q] = (int16_t)score;
			else
				A.out[q] = score;
			if (A.host_out)
				__builtin_nontemporal_store(score, &A.host_out[q]);
		}
	}
}

/* Packed triangular -> full symmetric (reference layout src/io/output.c:76-81), zero diagonal.
 * One thread per element of the full matrix: reads are gathers from the packed vector
 * (contiguous along i for fixed j), writes are fully coalesced rows. */
__global__ __launch_bounds__(256) void sa_k_expand_full(const int32_t *__restrict__ packed,
							  int32_t *__restrict__ full, int32_t num)
{
	const int64_t total = (int64_t)num * num;
	for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
	     e += (int64_t)gridDim.x * blockDim.x) {
		const int64_t r = e / num, c = e - r * num;
		int32_t v = 0;
		if (r != c) {
			const int64_t lo = r < c ? r : c, hi = r < c ? c : r;
			v = packed[hi * (hi - 1) / 2 + lo];
		}
		full[e] = v;
	}
}

/* The L-shaped shell of the full matrix owned by columns [ja, jb): rows [ja, jb) x cols [0, jb) (region A, row-major
 * first) and rows [0, ja) x cols [ja, jb) (region B).  Every element's pair has its larger index in [ja, jb), i.e.
 * belongs to the packed range tri(ja) .. tri(jb) that was just computed; packed[p - pbase] holds pair p. */
__global__ __launch_bounds__(256) void sa_k_expand_shell(const int32_t *__restrict__ packed, int64_t pbase,
							   int32_t *__restrict__ full, int32_t num, int32_t ja, int32_t jb)
{
	const int64_t na = (int64_t)(jb - ja) * jb, nb = (int64_t)ja * (jb - ja);
	for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < na + nb;
	     e += (int64_t)gridDim.x * blockDim.x) {
		int64_t r, c;
		if (e < na) {
			r = ja + e / jb;
			c = e % jb;
		} else {
			const int64_t f = e - na;
			r = f / (jb - ja);
			c = ja + f % (jb - ja);
		}
		int32_t v = 0;
		if (r != c) {
			const int64_t lo = r < c ? r : c, hi = r < c ? c : r;
			v = packed[hi * (hi - 1) / 2 + lo - pbase];
		}
		full[r * num + c] = v;
	}
}

} // namespace

hipError_t sa_launch_generic(int method, const SaGenericArgs &a, int blocks, hipStream_t s)
{
	switch (method) {
	case SA_METHOD_NW:
		hipLaunchKernelGGL(sa_k_pair_per_wave<SA_METHOD_NW>, dim3(blocks), dim3(256), 0, s, a);
		break;
	case SA_METHOD_GA:
		hipLaunchKernelGGL(sa_k_pair_per_wave<SA_METHOD_GA>, dim3(blocks), dim3(256), 0, s, a);
		break;
	case SA_METHOD_SW:
		hipLaunchKernelGGL(sa_k_pair_per_wave<SA_METHOD_SW>, dim3(blocks), dim3(256), 0, s, a);
		break;
	default:
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

const char *sa_generic_kernel_name(int method)
{
	static const char *names[] = { "sa_k_pair_per_wave<nw>", "sa_k_pair_per_wave<ga>", "sa_k_pair_per_wave<sw>" };
	return (method >= 0 && method < 3) ? names[method] : "?";
}

/* int16 exchange format back to the reference's s32 (sign extension), 8 scores per thread and pass */
__global__ __launch_bounds__(256) void sa_k_widen16(const int16_t *__restrict__ src, int32_t *__restrict__ dst, int64_t count,
						     int64_t nvec /* 16-byte groups (0 when a pointer is not 16-byte aligned) */)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
		const uint4 w = reinterpret_cast<const uint4 *>(src)[v];
		int4 lo, hi;
		lo.x = (int16_t)(w.x & 0xffffu), lo.y = (int16_t)(w.x >> 16), lo.z = (int16_t)(w.y & 0xffffu), lo.w = (int16_t)(w.y >> 16);
		hi.x = (int16_t)(w.z & 0xffffu), hi.y = (int16_t)(w.z >> 16), hi.z = (int16_t)(w.w & 0xffffu), hi.w = (int16_t)(w.w >> 16);
		reinterpret_cast<int4 *>(dst)[2 * v] = lo;
		reinterpret_cast<int4 *>(dst)[2 * v + 1] = hi;
	}
	for (int64_t k = (nvec << 3) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride)
		dst[k] = src[k];
}

hipError_t sa_launch_widen16(const int16_t *src, int32_t *dst, int64_t count, hipStream_t s)
{
	if (count <= 0)
		return hipSuccess;
	int64_t blocks = ((count >> 3) + 255) / 256;
	blocks = blocks < 1 ? 1 : blocks > 256 * 16 ? 256 * 16 : blocks;
	const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
	hipLaunchKernelGGL(sa_k_widen16, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, count, aligned ? count >> 3 : (int64_t)0);
	return hipGetLastError();
}

hipError_t sa_launch_expand_shell(const int32_t *packed, int64_t pbase, int32_t *full, int32_t num, int32_t ja, int32_t jb,
				  hipStream_t s)
{
	const int64_t total = (int64_t)(jb - ja) * jb + (int64_t)ja * (jb - ja);
	if (total <= 0)
		return hipSuccess;
	int64_t blocks = (total + 255) / 256;
	if (blocks > 256 * 16)
		blocks = 256 * 16;
	hipLaunchKernelGGL(sa_k_expand_shell, dim3((unsigned)blocks), dim3(256), 0, s, packed, pbase, full, num, ja, jb);
	return hipGetLastError();
}

hipError_t sa_launch_expand_full(const int32_t *packed, int32_t *full, int32_t num, hipStream_t s)
{
	const int64_t total = (int64_t)num * num;
	int64_t blocks = (total + 255) / 256;
	if (blocks > 256 * 16)
		blocks = 256 * 16;
	hipLaunchKernelGGL(sa_k_expand_full, dim3((unsigned)blocks), dim3(256), 0, s, packed, full, num);
	return hipGetLastError();
}

/* Widen-and-place (tile-interleaved sharding, sa_ctx_place_shares): the gathered dense shares -- every rank's scores in
 * tile order, int16 or s32 -- into the reference's packed order.  One workgroup per run of a tile (SaPlaceSeg): reads are
 * contiguous, writes land inside one arranged block of the column (<= 2048 rows = an 8 KB window the L2 merges), in row
 * order where the tile streamed in store order. */
template <typename T>
__global__ __launch_bounds__(256) void sa_k_place(const SaPlaceSeg *__restrict__ segs, int32_t nsegs, const T *__restrict__ shares,
						   int32_t *__restrict__ packed)
{
	/* One WAVE per run and pass (a run is at most a tile's rows; a workgroup per run was 240 000 workgroups of one
	 * iteration each for cfg 2 at 8 ranks -- 0.45 ms of dispatch).  A tile that is its own arranged block holds a
	 * permutation of the rows [pos0, pos0 + count): it is placed OUTPUT-driven -- a lane takes four consecutive rows,
	 * looks their positions up (posmap: one 16-byte load), gathers the four scores from the run (a 1-2 KB window) and
	 * stores 16 contiguous bytes.  Position-driven scattering made the L2 write partial lines (1.2 TB/s for the pass). */
	const int lane = threadIdx.x & 63;
	const int32_t wave = (int32_t)((blockIdx.x * 256 + threadIdx.x) >> 6), nwaves = (int32_t)(gridDim.x * 4);
	typedef int32_t i32x4 __attribute__((ext_vector_type(4), aligned(4)));
	constexpr int WIN = 2048; /* elements of a wave's LDS window = rows of the largest own-block tile (eight waves x 8 streams x 32) */
	__shared__ __attribute__((aligned(16))) T s_win[4 * WIN];
	for (int32_t k = wave; k < nsegs; k += nwaves) {
		const SaPlaceSeg sg = segs[k];
		const T *src = shares + sg.src;
		int32_t *dst = packed + sg.dst;
		if (sg.flags & 1) { /* map = posmap (row -> position), rows [pos0, pos0 + count) */
			/* A run is one tile's rows (<= 1024).  The run is copied into this wave's LDS window with coalesced 16-byte loads
			 * (runs are padded to multiples of 8 elements: SA_SHARE_PAD), the positions of four groups of four rows per lane
			 * are looked up while that copy is in flight, and the scores are then gathered from LDS: the texture path sees
			 * only whole cache lines (2-byte gathers from global memory kept the pass at 2.2 TB/s). */
			T *const win = s_win + (threadIdx.x >> 6) * WIN;
			if (sg.count > WIN) { /* (no tile is that large today: plain gathers) */
				for (int32_t q = lane; q < sg.count; q += 64)
					if (sg.pos0 + q >= sg.ia && sg.pos0 + q < sg.ib)
						dst[sg.pos0 + q] = (int32_t)src[sg.map[sg.pos0 + q] - sg.pos0];
				continue;
			}
			{
				constexpr int32_t q0 = 0;
				const int32_t n = sg.count, npad = (n + 7) & ~7;
				constexpr int PER = 16 / (int)sizeof(T); /* elements per 16-byte load */
				typedef T tvec __attribute__((ext_vector_type(16 / sizeof(T)), aligned(16)));
				for (int32_t e = PER * lane; e < npad; e += PER * 64)
					*reinterpret_cast<tvec *>(win + e) = *reinterpret_cast<const tvec *>(src + q0 + e);
				i32x4 pp[4], v[4];
				bool whole[4];
#pragma unroll
				for (int g = 0; g < 4; g++) {
					const int32_t q = q0 + 256 * g + 4 * lane;
					whole[g] = q + 4 <= sg.count;
					if (whole[g])
						pp[g] = *reinterpret_cast<const i32x4 *>(sg.map + sg.pos0 + q);
				}
				/* (a tile that is its own block: the positions of its rows are its own positions, pos0 + [0, count)) */
				const int32_t off = sg.pos0 + q0;
#pragma unroll
				for (int g = 0; g < 4; g++)
					if (whole[g])
						v[g] = i32x4{ (int32_t)win[pp[g].x - off], (int32_t)win[pp[g].y - off], (int32_t)win[pp[g].z - off],
							      (int32_t)win[pp[g].w - off] };
#pragma unroll
				for (int g = 0; g < 4; g++) {
					const int32_t q = q0 + 256 * g + 4 * lane, r = sg.pos0 + q;
					if (whole[g] && r >= sg.ia && r + 4 <= sg.ib) {
						*reinterpret_cast<i32x4 *>(dst + r) = v[g];
						continue;
					}
					for (int e = 0; e < 4 && q + e < sg.count; e++) /* a column whose range ends inside these four rows; the run's tail */
						if (r + e >= sg.ia && r + e < sg.ib)
							dst[r + e] = (int32_t)src[sg.map[r + e] - sg.pos0];
				}
			}
		} else { /* map = rowmap (position -> row) or null (store order) */
			for (int32_t p = lane; p < sg.count; p += 64) {
				const int32_t r = sg.map ? sg.map[sg.pos0 + p] : sg.pos0 + p;
				if (r >= sg.ia && r < sg.ib)
					dst[r] = (int32_t)src[p];
			}
		}
	}
}

hipError_t sa_launch_place(const SaPlaceSeg *segs, int32_t nsegs, const void *shares, int elem16, int32_t *packed, hipStream_t s)
{
	if (nsegs <= 0)
		return hipSuccess;
	const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)nsegs + 3) / 4, 256 * 8);
	if (elem16)
		hipLaunchKernelGGL(sa_k_place<int16_t>, dim3(blocks), dim3(256), 0, s, segs, nsegs, static_cast<const int16_t *>(shares), packed);
	else
		hipLaunchKernelGGL(sa_k_place<int32_t>, dim3(blocks), dim3(256), 0, s, segs, nsegs, static_cast<const int32_t *>(shares), packed);
	return hipGetLastError();
}

/* see sa_warm_kernels: the pair-per-wave, expand, widen and place kernels live in this translation unit */
hipError_t sa_warm_generic(void)
{
	hipFuncAttributes attr;
	return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sa_k_expand_full));
}
