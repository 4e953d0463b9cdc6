// Microbenchmark (development tool): v_pk_maximum3_f16 as a packed UNSIGNED 3-way max on gfx950.
// For bit patterns 0x0000..0x7c00 (non-negative f16, zero .. +inf) the f16 order is the u16 order, so the packed
// 3-operand f16 maximum is a two-lane max3_u16 -- if the instruction neither flushes denormals nor touches payloads.
// Part 1 checks that exhaustively over all pairs (every operand position, both halves); part 2 measures its issue cost
// next to v_pk_max_u16 and the shape the NW chain would use (add + max3 per register).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__device__ __forceinline__ uint32_t max3f(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t d;
	asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
	return d;
}

/* the same as two nested elementwise maxima on _Float16 pairs: the compiler selects the instruction itself */
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t max3b(uint32_t a, uint32_t b, uint32_t c)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
									  __builtin_bit_cast(f16x2, c)));
}

/* Eight dependent links in ONE asm statement: the compiler pads nothing inside a statement, so every link reads the
 * result of the instruction right before it with no wait state in between.  v[i] = max3(d[i], v[i], v[i-1]). */
__device__ __forceinline__ void chain8(uint32_t (&v)[8], const uint32_t (&d)[8], uint32_t left)
{
	asm("v_pk_maximum3_f16 %0, %8, %0, %16\n\t"
	    "v_pk_maximum3_f16 %1, %9, %1, %0\n\t"
	    "v_pk_maximum3_f16 %2, %10, %2, %1\n\t"
	    "v_pk_maximum3_f16 %3, %11, %3, %2\n\t"
	    "v_pk_maximum3_f16 %4, %12, %4, %3\n\t"
	    "v_pk_maximum3_f16 %5, %13, %5, %4\n\t"
	    "v_pk_maximum3_f16 %6, %14, %6, %5\n\t"
	    "v_pk_maximum3_f16 %7, %15, %7, %6"
	    : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
	    : "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]), "v"(d[4]), "v"(d[5]), "v"(d[6]), "v"(d[7]), "v"(left));
}

/* the builtin form in every operand position, both halves, every pair of patterns; and the unpadded chain: its eight
 * links against the same recurrence in u16 arithmetic (a link that read a stale register would differ) */
__global__ void check_forms(unsigned long long *bad, uint32_t limit)
{
	const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
	if (a > limit) return;
	unsigned long long nb = 0, nc = 0;
	for (uint32_t b = 0; b <= limit; b++) {
		const uint32_t m = a > b ? a : b;
		const uint32_t lo_hi = a | (b << 16), hi_lo = b | (a << 16), z = 0, mm = m | (m << 16);
		nb += max3b(lo_hi, hi_lo, z) != mm;
		nb += max3b(lo_hi, z, hi_lo) != mm;
		nb += max3b(z, lo_hi, hi_lo) != mm;
		nb += max3b(lo_hi, hi_lo, lo_hi) != mm;
		const uint32_t c = (a + b) >> 1;
		nb += max3b(c | (c << 16), lo_hi, hi_lo) != mm;
		nb += max3b(lo_hi, c | (c << 16), hi_lo) != mm;
		nb += max3b(lo_hi, hi_lo, c | (c << 16)) != mm;
		/* chain: registers and addends that rise and fall along the links, so the running maximum changes hands */
		uint32_t v[8], d[8], w[8];
		const uint32_t left = lo_hi;
		for (int i = 0; i < 8; i++) {
			const uint32_t x = (a * (uint32_t)(i + 3) + b * 7u) % (limit + 1u), y = (b * (uint32_t)(i + 5) + a * 11u + 13u * i) % (limit + 1u);
			v[i] = x | (y << 16);
			d[i] = y | (x << 16);
			if (i & 1) d[i] = (d[i] >> 1) & 0x7fff7fffu;
		}
		uint32_t pl = left & 0xffffu, ph = left >> 16;
		for (int i = 0; i < 8; i++) {
			uint32_t l = v[i] & 0xffffu, h = v[i] >> 16;
			const uint32_t dl = d[i] & 0xffffu, dh = d[i] >> 16;
			l = l > dl ? l : dl; l = l > pl ? l : pl;
			h = h > dh ? h : dh; h = h > ph ? h : ph;
			w[i] = l | (h << 16);
			pl = l; ph = h;
		}
		chain8(v, d, left);
		for (int i = 0; i < 8; i++) nc += v[i] != w[i];
	}
	if (nb) atomicAdd(bad, nb);
	if (nc) atomicAdd(bad + 1, nc);
}

__global__ void check(unsigned long long *bad, uint32_t limit)
{
	const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
	if (a > limit) return;
	unsigned long long nb = 0;
	for (uint32_t b = 0; b <= limit; b++) {
		const uint32_t m = a > b ? a : b;
		const uint32_t lo_hi = a | (b << 16), hi_lo = b | (a << 16), z = 0, mm = m | (m << 16);
		/* halves are independent: low = a vs b, high = b vs a */
		nb += max3f(lo_hi, hi_lo, z) != mm;
		nb += max3f(lo_hi, z, hi_lo) != mm;
		nb += max3f(z, lo_hi, hi_lo) != mm;
		nb += max3f(lo_hi, hi_lo, lo_hi) != mm;
		/* three distinct operands: c = (a + b) / 2 lies between */
		const uint32_t c = (a + b) >> 1;
		nb += max3f(c | (c << 16), lo_hi, hi_lo) != mm;
	}
	if (nb) atomicAdd(bad, nb);
}

constexpr int REP = 1500;
template <int MODE> __global__ __launch_bounds__(256) void rate(uint32_t *out, int seed)
{
	uint32_t v[8], d[8], w = threadIdx.x * 0x00010001u + seed, x = seed * 3;
	for (int q = 0; q < 8; q++) v[q] = (threadIdx.x + q * seed) & 0x3fff3fffu, d[q] = v[q] ^ 0x11;
	for (int r = 0; r < REP; r++) {
#pragma unroll
		for (int u = 0; u < 4; u++) {
#pragma unroll
			for (int q = 0; q < 8; q++) {
				if (MODE == 0) asm volatile("v_pk_max_u16 %0, %1, %0" : "+v"(v[q]) : "v"(w));
				if (MODE == 1) asm volatile("v_pk_maximum3_f16 %0, %1, %0, %2" : "+v"(v[q]) : "v"(w), "v"(x));
				if (MODE == 2) asm volatile("v_max3_u16 %0, %1, %0, %2" : "+v"(v[q]) : "v"(w), "v"(x));
				if (MODE == 3) { /* NW chain shape, u16: add, max, max (dependent chain through v[q-1]) */
					asm volatile("v_add_u32_e32 %0, %1, %2" : "=v"(d[q]) : "v"(w), "v"(v[(q + 7) & 7]));
					asm volatile("v_pk_max_u16 %0, %1, %0" : "+v"(v[q]) : "v"(d[q]));
					asm volatile("v_pk_max_u16 %0, %1, %0" : "+v"(v[q]) : "v"(v[(q + 7) & 7]));
				}
				if (MODE == 4) { /* NW chain shape, max3: add, max3 */
					asm volatile("v_add_u32_e32 %0, %1, %2" : "=v"(d[q]) : "v"(w), "v"(v[(q + 7) & 7]));
					asm volatile("v_pk_maximum3_f16 %0, %1, %0, %2" : "+v"(v[q]) : "v"(d[q]), "v"(v[(q + 7) & 7]));
				}
				if (MODE == 5) { /* max3 chain with the adds hoisted (8 adds, then 8 dependent max3) */
					asm volatile("v_add_u32_e32 %0, %1, %2" : "=v"(d[q]) : "v"(w), "v"(v[(q + 7) & 7]));
				}
			}
			if (MODE == 5) {
#pragma unroll
				for (int q = 0; q < 8; q++)
					asm volatile("v_pk_maximum3_f16 %0, %1, %0, %2" : "+v"(v[q]) : "v"(d[q]), "v"(v[(q + 7) & 7]));
			}
		}
	}
	uint32_t s = 0;
	for (int q = 0; q < 8; q++) s += v[q] + d[q];
	out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

/* The hoisted shape again with the register count as a parameter, and with the adds paired: two neighbouring registers
 * hold four u16 fields that never carry (the packing invariant), so one v_lshl_add_u64 with shift 0 on the even-aligned
 * pair does both adds. Odd NR keeps one plain add for the last register. PAIRED adds read v[q] where the plain rows read
 * v[q-1] (a pair has to be two neighbours); both are hoisted in front of the chain, so the issue stream is the same. */
template <int NR, bool PAIRED> __global__ __launch_bounds__(256) void rate_chain(uint32_t *out, int seed)
{
	uint32_t v[NR], d[NR], w = threadIdx.x * 0x00010001u + seed;
	for (int q = 0; q < NR; q++) v[q] = (threadIdx.x + q * seed) & 0x3fff3fffu, d[q] = v[q] ^ 0x11;
	const uint64_t ww = ((uint64_t)(w ^ 0x5) << 32) | w;
	for (int r = 0; r < REP; r++) {
#pragma unroll
		for (int u = 0; u < 4; u++) {
			if (PAIRED) {
#pragma unroll
				for (int q = 0; q + 1 < NR; q += 2) {
					uint64_t s, x = ((uint64_t)v[q + 1] << 32) | v[q];
					asm volatile("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(s) : "v"(x), "v"(ww));
					d[q] = (uint32_t)s, d[q + 1] = (uint32_t)(s >> 32);
				}
				if (NR & 1) asm volatile("v_add_u32_e32 %0, %1, %2" : "=v"(d[NR - 1]) : "v"(w), "v"(v[NR - 1]));
			} else {
#pragma unroll
				for (int q = 0; q < NR; q++)
					asm volatile("v_add_u32_e32 %0, %1, %2" : "=v"(d[q]) : "v"(w), "v"(v[(q + NR - 1) % NR]));
			}
#pragma unroll
			for (int q = 0; q < NR; q++)
				asm volatile("v_pk_maximum3_f16 %0, %1, %0, %2" : "+v"(v[q]) : "v"(d[q]), "v"(v[(q + NR - 1) % NR]));
		}
	}
	uint32_t s = 0;
	for (int q = 0; q < NR; q++) s += v[q] + d[q];
	out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

/* The paired 8-register chain once more with its eight maxima as one asm statement (chain8): the separate statements above
 * get a wait state (s_nop 0) from the compiler between every two links, the single statement gets none. */
__global__ __launch_bounds__(256) void rate_chain_unpadded(uint32_t *out, int seed)
{
	uint32_t v[8], d[8], w = threadIdx.x * 0x00010001u + seed;
	for (int q = 0; q < 8; q++) v[q] = (threadIdx.x + q * seed) & 0x3fff3fffu, d[q] = v[q] ^ 0x11;
	const uint64_t ww = ((uint64_t)(w ^ 0x5) << 32) | w;
	for (int r = 0; r < REP; r++) {
#pragma unroll
		for (int u = 0; u < 4; u++) {
#pragma unroll
			for (int q = 0; q + 1 < 8; q += 2) {
				uint64_t s, x = ((uint64_t)v[q + 1] << 32) | v[q];
				asm volatile("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(s) : "v"(x), "v"(ww));
				d[q] = (uint32_t)s, d[q + 1] = (uint32_t)(s >> 32);
			}
			chain8(v, d, v[7]);
		}
	}
	uint32_t s = 0;
	for (int q = 0; q < 8; q++) s += v[q] + d[q];
	out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int MODE, int NR = 8, bool PAIRED = false> int run(const char *name, double per)
{
	uint32_t *out;
	CHECK(hipMalloc(&out, 4 * 256 * 8 * 256));
	printf("%-44s", name);
	for (int bpc : { 1, 2, 4, 8 }) {
		hipEvent_t e0, e1;
		CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
		void (*kern)(uint32_t *, int);
		if constexpr (MODE < 6) kern = rate<MODE>; else if constexpr (MODE == 7) kern = rate_chain_unpadded; else kern = rate_chain<NR, PAIRED>;
		hipLaunchKernelGGL(kern, dim3(256 * bpc), dim3(256), 0, 0, out, 3);
		CHECK(hipEventRecord(e0, 0));
		hipLaunchKernelGGL(kern, dim3(256 * bpc), dim3(256), 0, 0, out, 3);
		CHECK(hipEventRecord(e1, 0));
		CHECK(hipDeviceSynchronize());
		float ms = 0.f;
		CHECK(hipEventElapsedTime(&ms, e0, e1));
		printf("  %6.3f ns", (double)ms * 1e6 / ((double)REP * 4 * 8 * per * bpc));
	}
	printf("\n");
	(void)hipFree(out);
	return 0;
}

int main()
{
	unsigned long long *bad, h = 0;
	CHECK(hipMalloc(&bad, 8));
	CHECK(hipMemset(bad, 0, 8));
	const uint32_t limit = 0x7c00;
	hipLaunchKernelGGL(check, dim3((limit + 256) / 256), dim3(256), 0, 0, bad, limit);
	CHECK(hipDeviceSynchronize());
	CHECK(hipMemcpy(&h, bad, 8, hipMemcpyDeviceToHost));
	printf("v_pk_maximum3_f16 vs unsigned max over all pairs of 0x0000..0x%04x, 5 operand arrangements, both halves: %llu mismatches\n", limit, h);
	unsigned long long *bad2, h2[2] = { 0, 0 };
	CHECK(hipMalloc(&bad2, 16));
	CHECK(hipMemset(bad2, 0, 16));
	hipLaunchKernelGGL(check_forms, dim3((limit + 256) / 256), dim3(256), 0, 0, bad2, limit);
	CHECK(hipDeviceSynchronize());
	CHECK(hipMemcpy(h2, bad2, 16, hipMemcpyDeviceToHost));
	printf("builtin form (nested elementwise maximum on _Float16 pairs) vs unsigned max, the same pairs, 7 operand arrangements, both halves: %llu mismatches\n", h2[0]);
	printf("8 dependent links in one asm statement (no wait states between them) vs the u16 recurrence, the same pairs: %llu mismatching links\n", h2[1]);
	printf("host-timed ns per wave64 instruction (or per register step of a chain) and SIMD; columns = 1,2,4,8 waves/SIMD\n");
	run<0>("v_pk_max_u16", 1);
	run<1>("v_pk_maximum3_f16", 1);
	run<2>("v_max3_u16", 1);
	run<3>("NW register step: add + 2 v_pk_max_u16", 1);
	run<4>("NW register step: add + v_pk_maximum3_f16", 1);
	run<5>("NW register step: adds hoisted, max3 chain", 1);
	run<6, 8, false>("  the same, 8 registers (parametrised)", 1);
	run<6, 8, true>("  8 registers, 4 v_lshl_add_u64", 1);
	run<7>("  8 registers, 4 v_lshl_add_u64, maxima unpadded", 1);
	run<6, 7, false>("  the same, 7 registers", 7.0 / 8);
	run<6, 7, true>("  7 registers, 3 v_lshl_add_u64 + 1 add", 7.0 / 8);
	return h != 0 || h2[0] != 0 || h2[1] != 0;
}
