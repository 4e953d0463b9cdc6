/*
 * sa_wave_sweep.h -- one pair per wavefront: the helpers of the score sweep (sa_wave_sweep.inc), which sa_k_pair_per_wave
 * (sa_generic.hip) and sa_k_self (sa_normalize.hip) include (gfx950, wave64; device code).
 */
#ifndef SA_WAVE_SWEEP_H
#define SA_WAVE_SWEEP_H

#include "sa_internal.h"

namespace {

constexpr int32_t SCORE_MIN = SA_SCORE_MIN; /* reference src/bio/align.h:19 */

__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

/* packed index -> (i,j), i<j : largest j with j(j-1)/2 <= p
 * (what the reference does by binary search, src/bio/kernels.cu:17-30) */
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

/* value shifted in from lane-1 (DPP wave_shr:1 -- full 64-lane shift, bound_ctrl off: lane 0 keeps `v` and overrides it
 * afterwards) */
__device__ __forceinline__ int32_t from_left(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ int32_t wave_max(int32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v = imax(v, __shfl_xor(v, d, 64));
	return v;
}

} // namespace

#endif /* SA_WAVE_SWEEP_H */
