/*
 * sa_systolic_pk.inc -- packed-u16 streaming systolic wave kernels (gfx950, wave64): the fast path for column
 * sequences of up to 1024 residues.  Included by sa_systolic_pk_{nw,ga,sw}.hip (8-lane groups), sa_systolic_pk16_{nw,ga,sw}.hip
 * (16-lane groups, K <= 44) and sa_systolic_pk16hi_{nw,ga,sw}.hip (16-lane groups, K >= 45): SA_SYS_METHOD, SA_PK_G,
 * SA_PK16_PART -- one code object per method, group width and K range.
 *
 * Same mapping as sa_systolic_kernel.inc (read that header first): lane groups of G = 8 lanes (two interleaved groups
 * per DPP row; columns <= 192, K <= 24) or G = 16 lanes (one group per DPP row; 193..1024 columns, K = 13..64), K DP
 * columns per lane in VGPRs, the rows are the encoded store streamed through a small LDS token ring, one DPP move per
 * step, sequence boundaries cost no per-cell work.  What is different:
 *
 * Two column sequences per register.  Every DP register holds the same column slot of TWO column sequences jA, jB
 * (consecutive columns of the launch's class) as u16 halves, so one v_pk_max_u16 advances two cells.  Measured on
 * gfx950 (profiles/r02_microbench_*): every VOP3 / SDWA / DPP / VOP3P instruction costs ~4.1 SIMD cycles per wave64,
 * a plain 32-bit VOP2 add / sub ~2.5, independent of occupancy (>= 2 waves) and of dependencies -- the s32 kernels
 * (v_add_u32_sdwa + v_max3_i32 = 8.2 cycles per NW cell) run at ~85 % of that bound, so the lever is fewer and
 * cheaper instructions per cell:
 *   NW  nw.c:29-35   d = Vdiag + S'  (v_add_u32 on both halves at once)   V = pk_max(pk_max(d, V), Vleft)
 *                    10.7 cycles per TWO cells (5.35 / cell)
 *   GA  ga.c:46-63   y = pk_max(V, Y); d = Vdiag + S'; m = pk_max(pk_max(d, y), x); V = m - |q|; x = pk_max(V, x)
 *                    21.4 cycles per two cells (10.7 / cell, s32 kernel: 18.9)
 * The 32-bit add / sub act on both halves because the halves are UNSIGNED and never carry or borrow: all values live
 * in [floor, 65535 - S'max], the profile entries S' = S + const are >= 0 (host-checked, else the s32 kernels run).
 *
 * Two diagonal adds per instruction (NW, SA_PK_PAIRED_ADDS).  The same argument one level up: two neighbouring registers
 * are four u16 fields of one 64-bit integer, and by the range predicate above no field of Vdiag + S' exceeds 65535, so
 * nothing carries from a field into the next one -- neither inside a register nor from the high half of a register into
 * the low half of its neighbour.  One v_lshl_add_u64 (shift 0; operands are even-aligned VGPR pairs) therefore makes the
 * diagonal adds of the columns q, q + 1 of a lane: NW keeps its left neighbour's value in the register below column 0
 * (X[0] = the value moved in from the previous lane, X[q + 1] = V[q]), the pairs are (X[q], X[q + 1]) for even q against
 * components 0/1 or 2/3 of a 16-byte profile part, and odd K keeps one plain add for its last column.  The adds of a
 * step run before its DPP move, while X[0] still holds the previous step's left value -- the diagonal input of column
 * 0 -- so the two alternating left-neighbour registers of the other methods are one here.  (Bubble rows may wrap as
 * before; a carry out of such a field lands in a cell of the same bubble row of the same lane, which is never stored.)
 * The instruction issues like every other VOP3 here (tools/microbench/valu_rates.hip, row v_lshl_add_u64), and the step
 * with it is 9.9 % faster on cfg 2 than with two plain adds (DESIGN.md 4.1 / 4.2, profiles/nw_step_ab_parent.txt).
 * Gotoh and SW make their diagonal adds just in time inside the chain and keep the 32-bit add.
 *
 * Three-way maxima in one instruction (8-lane groups).  gfx950 has v_pk_maximum3_f16, and on the bit patterns
 * 0x0000..0x7c00 the f16 order is the unsigned order: with all values <= SA_PK_F16_MAX = 0x7bff the instruction is a
 * packed max3_u16 (bit-exact, checked exhaustively by tools/microbench/max3_f16.hip; same issue cost as v_pk_max_u16):
 *   NW  V = max3(d, V, Vleft)                                          6.6 cycles per two cells (3.3 / cell)
 *   GA  y = pk_max(V, Y); m = max3(d, y, x); V = m - |q|; x = pk_max(V, x)          17.3 (8.65 / cell)
 *   SW  y = max3(V, Y, floor); m = max3(d, y, x); best = max3(best, m, m') per two columns;  ...   21.9 (10.9 / cell)
 * Values past the end of a stream (bubbles) may wrap into NaN patterns; like the wrapped u16 values of the two-way
 * form they only ever meet other bubble rows and are never stored.  The 16-lane kernels are compiled in BOTH forms
 * (template parameter F16) and the launch picks per class: three-way where the class's values fit 0x7bff (host:
 * sa_limits.cpp, pk16_f16_kmax -- up to K = SA_PK16_F16_KMAX), the two-way v_pk_max_u16 form with the full u16 range
 * where they do not (many frame shifts in flight because the store holds very short sequences, or K > 52).
 *
 * Sliding frame instead of a growing baseline.  The s32 kernels raise the injected baseline by DELTA per sequence;
 * here the baseline BASE is constant and, at the step a terminator ENTERS a group's first lane, every lane of that
 * group lowers all its DP registers by DELTA (exec-masked, on the rare event path: one v_pk_sub_u16 with clamp each).
 * A uniform shift commutes with max and with adding constants, so the rows of the previous sequence that are still
 * travelling through the group stay exact relative to each other, and everything older than the new sequence now
 * loses every max against BASE -- the reference's border initialisation (nw.c:14-20, ga.c:23-38).  A per-lane frame
 * counter F (shifts so far) turns the u16 captured at the group's last lane back into the value the s32 kernels
 * capture (v - BASE + F * DELTA), so the epilogue is theirs.  A value is shifted at most `live` = 1 + (G-1)/(Lmin+1) times
 * before it is captured (terminators are Lmin + 1 positions apart at least, Lmin = the store's shortest sequence; host:
 * pk_live): BASE = live * DELTA + margins, so a live value
 * is never clamped; what saturates at 0 is stale and has lost against the current sequence long before.
 *
 * LDS.  Profile: rows = residue codes (+ SEP, NOP: all zero), u16 pairs {S'(a, A[c]), S'(a, B[c])}, 4 K bytes per
 * distinct column holder, laid out [row][16-byte part][copy][slot]: a part spans 256 bytes = all 64 banks, and the 16
 * lanes of a ds_read_b128 phase hit 16 distinct 4-bank windows whatever rows they read -- with 16-lane groups because
 * they are 16 different slots, with 8-lane groups because the two interleaved groups of a DPP row (same slots) read
 * their own copy.  The profile (26 KB at K = 13..16) is shared by the SA_PK_WPB waves of a workgroup.  Tokens: u16 profile-row offsets in a per-group ring (duplicated, no wrap); a lane
 * reads ONE token per step with an immediate offset two steps ahead of its use -- no window registers, no
 * per-step address arithmetic, and the row address is a plain v_add_u32.  (NW, 8-lane groups, K <= 16, full tiles of an
 * arranged level: no ring at all -- the row offsets come from the level's row streams in global memory straight into
 * registers, sixteen per lane and block; SA_PK_REG_TOKENS, see REGT in pk_tile.)
 *
 * Tiles.  A workgroup-tile = (column pair, SA_PK_WPB * 8 row streams of up to A.chunk sequences).  Rows run over the
 * union of the two columns' row ranges; a score is stored only where its pair belongs to the packed range.  Tiles are
 * numbered largest first (full tiles, then the partial ones by size).  A full tile streams an ARRANGED copy of its rows
 * (sa_plan.cpp: sa_arrange_rows) in which the k-th sequences of a wave's streams have equal lengths wherever the
 * block has enough of them: their terminators share one event step and the streams end together.
 */
#include "sa_internal.h"
#include <atomic>
#include <type_traits>
#if !defined(SA_PK_G) || (SA_PK_G != 8 && SA_PK_G != 16)
#error "define SA_PK_G (8 or 16) before including sa_systolic_pk.inc"
#endif
#if SA_PK_G == 16 && !defined(SA_PK16_PART)
#error "define SA_PK16_PART (0: K = 13..44, 1: K = 45..64) before including sa_systolic_pk.inc with SA_PK_G 16"
#endif

/* A score goes out with a non-temporal store when the destination is host memory (A.out_nt: the kernel is storing
 * straight into the page-locked host matrix): with ordinary stores ~0.5 ms of posted writes were still sitting in the
 * L2s when the last kernel of cfg 2 ended.  In device memory ordinary stores let the L2 merge partial lines. */
#define SA_PK_STORE(nt, v, p)                          \
	do {                                           \
		if (nt) {                              \
			asm volatile(""); /* keeps the two stores apart: merged, they lose the nt bit */ \
			__builtin_nontemporal_store((v), (p)); \
		} else                                 \
			*(p) = (v);                    \
	} while (0)

#ifndef SA_PK_OPAQUE_TOKEN
#define SA_PK_OPAQUE_TOKEN 1
#endif
#ifndef SA_PK_PAIRED_ADDS
#define SA_PK_PAIRED_ADDS 1 /* NW: one v_lshl_add_u64 for the diagonal adds of two neighbouring columns (0: two v_add_u32) */
#endif
#ifndef SA_PK_CHAINED_MAX3
#define SA_PK_CHAINED_MAX3 1 /* NW: the step's dependent maxima as asm statements of up to eight links, no wait states between them (0: one statement per link) */
#endif
#ifndef SA_PK_QUIET_BLOCKS
#define SA_PK_QUIET_BLOCKS 0 /* measured slower, see do_block */
#endif

namespace {

extern __shared__ __attribute__((aligned(256))) uint8_t sa_pk_lds[];

constexpr int CH = SA_SYS_CHUNK;
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t pkmax(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pksubsat(uint32_t a, uint32_t b) /* v_pk_sub_u16 clamp: saturates at 0 */
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
/* Three-way packed max.  F16: v_pk_maximum3_f16 on the u16 bit patterns -- for patterns 0x0000..0x7c00 (the
 * non-negative halves, +0 .. +inf) the f16 order IS the unsigned order, and the instruction returns one of its operands
 * bit for bit (no flush, no canonicalisation: tools/microbench/max3_f16.hip checks every pair of patterns in every
 * operand position).  One VOP3P instead of two: the kernels that use it keep all values <= SA_PK_F16_MAX. */
template <bool F16> __device__ __forceinline__ uint32_t pkmax3(uint32_t a, uint32_t b, uint32_t c)
{
	if (F16) {
		uint32_t d;
		asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
		return d;
	}
	return pkmax(pkmax(a, b), c);
}
#if SA_PK_CHAINED_MAX3
/* N = 1..8 links of NW's dependent chain V[i] = max3(d[i], V[i], V[i - 1]) (V[-1] = left) as ONE asm statement.  The compiler
 * puts a wait state (s_nop 0) between a v_pk_maximum3_f16 and an adjacent instruction that reads its result: behind inline
 * asm because any asm result may be a partial-register (destination-select) write, and behind the same instruction selected
 * from __builtin_elementwise_maximum just as well (tried: 12 of the 13 pads of a K = 14 step stay, DESIGN.md 4.2).  The
 * instruction writes its whole destination register and the hardware needs no such state: tools/microbench/max3_f16.hip
 * runs eight links back to back at one wave per SIMD over every pair of patterns against the u16 recurrence.  The compiler
 * does not look inside a statement, so the chain is written as statements of eight links: K = 14 keeps 1 pad of 13. */
template <int N> __device__ __forceinline__ void pkmax3_chain(uint32_t *V, const uint32_t *d, uint32_t left)
{
	static_assert(N >= 1 && N <= 8, "one statement holds up to eight links");
#define SA_LK0 "v_pk_maximum3_f16 %[v0], %[d0], %[v0], %[l]"
#define SA_LK(i, p) "\n\tv_pk_maximum3_f16 %[v" #i "], %[d" #i "], %[v" #i "], %[v" #p "]"
#define SA_VO(i) [v##i] "+v"(V[i])
#define SA_DI(i) [d##i] "v"(d[i])
	if constexpr (N == 1)
		asm(SA_LK0 : SA_VO(0) : SA_DI(0), [l] "v"(left));
	else if constexpr (N == 2)
		asm(SA_LK0 SA_LK(1, 0) : SA_VO(0), SA_VO(1) : SA_DI(0), SA_DI(1), [l] "v"(left));
	else if constexpr (N == 3)
		asm(SA_LK0 SA_LK(1, 0) SA_LK(2, 1) : SA_VO(0), SA_VO(1), SA_VO(2) : SA_DI(0), SA_DI(1), SA_DI(2), [l] "v"(left));
	else if constexpr (N == 4)
		asm(SA_LK0 SA_LK(1, 0) SA_LK(2, 1) SA_LK(3, 2)
		    : SA_VO(0), SA_VO(1), SA_VO(2), SA_VO(3)
		    : SA_DI(0), SA_DI(1), SA_DI(2), SA_DI(3), [l] "v"(left));
	else if constexpr (N == 5)
		asm(SA_LK0 SA_LK(1, 0) SA_LK(2, 1) SA_LK(3, 2) SA_LK(4, 3)
		    : SA_VO(0), SA_VO(1), SA_VO(2), SA_VO(3), SA_VO(4)
		    : SA_DI(0), SA_DI(1), SA_DI(2), SA_DI(3), SA_DI(4), [l] "v"(left));
	else if constexpr (N == 6)
		asm(SA_LK0 SA_LK(1, 0) SA_LK(2, 1) SA_LK(3, 2) SA_LK(4, 3) SA_LK(5, 4)
		    : SA_VO(0), SA_VO(1), SA_VO(2), SA_VO(3), SA_VO(4), SA_VO(5)
		    : SA_DI(0), SA_DI(1), SA_DI(2), SA_DI(3), SA_DI(4), SA_DI(5), [l] "v"(left));
	else if constexpr (N == 7)
		asm(SA_LK0 SA_LK(1, 0) SA_LK(2, 1) SA_LK(3, 2) SA_LK(4, 3) SA_LK(5, 4) SA_LK(6, 5)
		    : SA_VO(0), SA_VO(1), SA_VO(2), SA_VO(3), SA_VO(4), SA_VO(5), SA_VO(6)
		    : SA_DI(0), SA_DI(1), SA_DI(2), SA_DI(3), SA_DI(4), SA_DI(5), SA_DI(6), [l] "v"(left));
	else
		asm(SA_LK0 SA_LK(1, 0) SA_LK(2, 1) SA_LK(3, 2) SA_LK(4, 3) SA_LK(5, 4) SA_LK(6, 5) SA_LK(7, 6)
		    : SA_VO(0), SA_VO(1), SA_VO(2), SA_VO(3), SA_VO(4), SA_VO(5), SA_VO(6), SA_VO(7)
		    : SA_DI(0), SA_DI(1), SA_DI(2), SA_DI(3), SA_DI(4), SA_DI(5), SA_DI(6), SA_DI(7), [l] "v"(left));
#undef SA_LK0
#undef SA_LK
#undef SA_VO
#undef SA_DI
}
template <int K, int Q0 = 0> __device__ __forceinline__ void pkmax3_chain_all(uint32_t (&V)[K], const uint32_t (&d)[K], uint32_t left)
{
	if constexpr (Q0 < K) {
		constexpr int N = K - Q0 < 8 ? K - Q0 : 8;
		pkmax3_chain<N>(&V[Q0], &d[Q0], Q0 ? V[Q0 ? Q0 - 1 : 0] : left);
		pkmax3_chain_all<K, Q0 + N>(V, d, left);
	}
}
#endif
/* Two diagonal adds in one instruction: (hi:lo) + (phi:plo) as ONE 64-bit integer add (v_lshl_add_u64, shift 0) on
 * even-aligned register pairs.  Exact for the same reason the 32-bit add is (see the header): no u16 field of a live
 * value carries, so nothing crosses from a register's high half into its neighbour's low half either. */
__device__ __forceinline__ void pkadd2(uint32_t lo, uint32_t hi, uint32_t plo, uint32_t phi, uint32_t &dlo, uint32_t &dhi)
{
	const uint64_t x = ((uint64_t)hi << 32) | lo, p = ((uint64_t)phi << 32) | plo;
	uint64_t d;
	asm("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(d) : "v"(x), "v"(p));
	dlo = (uint32_t)d;
	dhi = (uint32_t)(d >> 32);
}
__device__ __forceinline__ uint32_t pk2(uint32_t v) { return (v & 0xffffu) | (v << 16); }
__device__ __forceinline__ uint32_t comp(const uint4 &w, int k) { return k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w; }

/* value of the previous lane of the group; the group's first lane has no source and keeps `lead`.  G = 8: the two groups of
 * a DPP row are interleaved (even / odd lanes), the previous lane is two lanes away; G = 16: one group per DPP row */
template <int G> __device__ __forceinline__ uint32_t shift_in(uint32_t lead, uint32_t src)
{
	if (G == 8)
		return (uint32_t)__builtin_amdgcn_update_dpp((int)lead, (int)src, 0x112, 0xf, 0xf, false);
	return (uint32_t)__builtin_amdgcn_update_dpp((int)lead, (int)src, 0x111, 0xf, 0xf, false);
}

/* A pointer that is wave-uniform by construction, made so for the compiler.  The value goes through integers, and an
 * integer cast back to a plain pointer is a FLAT pointer: loads through it are flat_load, which count on the LDS
 * counter as well -- every wait for a profile row in the main loop then also waits for the row-stream prefetch in
 * flight (+10 % per step, measured).  So the result is cast in the GLOBAL address space, where all of these live. */
template <typename T> __device__ __forceinline__ T *uniform_ptr(T *p)
{
	const uint64_t v = reinterpret_cast<uint64_t>(p);
	const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
	typedef __attribute__((address_space(1))) T *global_ptr;
	return (T *)reinterpret_cast<global_ptr>(((uint64_t)hi << 32) | lo);
}

/* a load whose address is wave-uniform, by construction: the tile geometry (the class block of a bundle launch points into
 * global memory the compiler cannot prove unwritten; as vector loads these values and everything derived from them would
 * sit in VGPRs, +50 per kernel) */
__device__ __forceinline__ int32_t uload(const int32_t *p) { return __builtin_amdgcn_readfirstlane(*p); }

template <int METHOD, int G, int K, bool F16>
__device__ __forceinline__ void pk_tile(const SaSysArgs &A, const int32_t t_raw, const int32_t ntiles)
{
	static_assert(G == 8 || G == 16, "packed kernels: 8- or 16-lane groups");
	constexpr int NG = 64 / G, WPB = sa_pk_wpb(METHOD, G, K), NGW = NG * WPB; /* (eight waves around one profile where four leave SIMD slots empty: sa_shapes.h) */
	/* F16: all values <= SA_PK_F16_MAX (host: pk_setup), three-way maxima in one op.  8-lane groups always; 16-lane
	 * groups where the store's shortest sequence keeps few enough frame shifts in flight (else the two-way u16 form) */
	constexpr int W = G * K;
	constexpr int PARTS = (K + 3) / 4;      /* 16-byte parts of a lane's profile slot (4 column slots = 4 u16 pairs each) */
	constexpr int NSLOT = G;      /* distinct column holders                                                   */
	constexpr int COPIES = 16 / G; /* G = 8: one copy per lane parity; G = 16: the 16 lanes of a phase are 16 slots  */
	/* two copies of every part, one per lane parity (the two interleaved groups of a DPP row), 128 bytes = 32 banks
	 * apart: the 16 lanes of a ds_read_b128 phase -- 8 slots x 2 parities -- hit 16 distinct 4-bank windows whatever
	 * rows they read (rows and parts are multiples of 256 bytes = all 64 banks apart) */
	constexpr int PARTSTRIDE = COPIES * NSLOT * 16;
	static_assert(PARTSTRIDE == 256, "a part spans all 64 banks");
	constexpr int ROWSTRIDE = PARTS * PARTSTRIDE;
	constexpr int PROF_BYTES = SA_CODE_ROWS * ROWSTRIDE;
	/* token of a row = its offset in the profile, in bytes while that fits u16, else in units of 256 bytes (rows are
	 * multiples of PARTSTRIDE = 256 apart): the row address is then one v_lshl_add_u32 instead of one v_add_u32 */
	constexpr int TSHIFT = (SA_CODE_ROWS - 1) * ROWSTRIDE < 65536 ? 0 : 8;
	constexpr uint32_t TUNIT = (uint32_t)ROWSTRIDE >> TSHIFT;
	static_assert((SA_CODE_ROWS - 1) * TUNIT < 65536, "the token of a profile row must fit u16");
	/* LDS (dynamic, carved here: the bundle kernel calls several instantiations of this function and the LDS of
	 * a workgroup is that of the largest K it may meet, not their sum): scores, rings, then the profile */
	uint8_t *const s_prof = sa_pk_lds + sa_pk_lds_fixed(G, WPB);
	static_assert(PROF_BYTES + sa_pk_lds_fixed(G, WPB) == sa_pk_lds_bytes(METHOD, G, K), "host and kernel agree on the LDS of a class");
	/* scores leaving the pipeline: [half][group][sequence]; the staged substitution matrix shares the storage (it is
	 * only read by the profile build, which ends before the first score leaves) */
	constexpr int OUT_HALFS = 2 * NG * CH; /* int16 per wave: scores relative to their own sequence's baseline */
	static_assert(WPB * OUT_HALFS * 2 >= SA_SUB_DIM * SA_SUB_DIM, "the staged matrix must fit the score storage");
	int16_t *const s_out_all = reinterpret_cast<int16_t *>(sa_pk_lds);
	/* token ring per lane group: RING stream positions as u16 profile-row offsets, stored twice (i and i + RING) so
	 * that a lane's run of 18 consecutive positions never wraps */
	constexpr int RING = 64;
	constexpr int GSTRIDE = 2 * RING + 16; /* u16; +16 = 8 banks: the 8 groups' 5-bank read windows never overlap */
	uint16_t *const s_ring_all = reinterpret_cast<uint16_t *>(sa_pk_lds + WPB * OUT_HALFS * 2);
	static_assert(WPB * OUT_HALFS * 2 + WPB * NG * GSTRIDE * 2 == sa_pk_lds_fixed(G, WPB), "LDS carve");
	static_assert(sa_pk_lds_fixed(G, WPB) % 256 == 0, "the profile starts on a 256-byte boundary: a part spans all 64 banks");

	/* (opaque to the optimiser: the bundle kernel calls up to eight instantiations of this function from one persistent
	 * loop, and per-lane values that depend only on the lane id would all be hoisted out of that loop and stay live
	 * across every instantiation -- 180 VGPRs instead of 104 for K = 9..16) */
	int lane_id = threadIdx.x;
	asm volatile("" : "+v"(lane_id));
	const int lane = lane_id & 63;
	const int wv = __builtin_amdgcn_readfirstlane(lane_id >> 6);
	int16_t *s_out = s_out_all + wv * OUT_HALFS;
	uint16_t *s_ring = s_ring_all + wv * (NG * GSTRIDE);
	const int lig = G == 8 ? (lane & 15) >> 1 : lane & 15;              /* lane in group                       */
	const int grp = G == 8 ? (lane >> 4) * 2 + (lane & 1) : lane >> 4;  /* group of the wave (G = 8: row x parity) */
	const int copy = G == 8 ? lane & 1 : 0;                             /* profile copy this lane reads         */
	const bool leader = lig == 0;

	/* ---- which workgroup-tile: (column pair, block of NGW * chunk rows) ---- */
	const bool active = t_raw < ntiles;            /* surplus workgroups recompute the last tile and store nothing */
	const int32_t t = active ? t_raw : ntiles - 1;
	/* Tiles are numbered largest first: the FULL tiles of all column pairs (tprefix counts those), then the partial
	 * last tiles of the pairs that have one, by decreasing size (their pairs are listed behind tprefix) -- the launch
	 * tapers off instead of ending on a few full tiles. */
	const int32_t npairs = (A.ncols + 1) >> 1;
	const int32_t nfull = uload(A.tprefix + npairs);
	/* (the column pair of the tile comes with the tile from the launch's list: a binary search over tprefix here was a
	 * dozen dependent global loads, most of the prologue's 10 us) */
	const int32_t lo = A.tile_pair;
	const int32_t jh[2] = { uload(A.jlist + 2 * lo), uload(A.jlist + (2 * lo + 1 < A.ncols ? 2 * lo + 1 : 2 * lo)) };
	const bool dup = 2 * lo + 1 >= A.ncols; /* odd column count: the last column is paired with itself, stored once */
	int64_t tri[2];
	int32_t ia[2], ib[2], offj[2], nh[2], pad[2];
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const int32_t j = jh[h];
		tri[h] = (int64_t)j * (j - 1) / 2;
		const int64_t a = A.start > tri[h] ? A.start - tri[h] : 0;
		const int64_t jb = A.row_end && A.row_end < j ? A.row_end : j; /* (a search context's row bound) */
		const int64_t b = A.end - tri[h] < jb ? A.end - tri[h] : jb;
		ia[h] = (int32_t)a;
		ib[h] = (int32_t)(b > a ? b : a);
		offj[h] = uload(A.off + j);
		nh[h] = uload(A.off + j + 1) - offj[h] - 1;
		pad[h] = W - nh[h]; /* the sequence is right-aligned over the W column slots */
	}
	int32_t ra = ia[0] < ia[1] ? ia[0] : ia[1], rb = ib[0] > ib[1] ? ib[0] : ib[1];
	if (A.piece) { /* remainder tiles: this class runs the rows of its window of the pair (sa_shapes.h: sa_pk_piece_window) */
		sa_pk_piece_window(ra, rb, (NGW * A.chunk) << (A.piece & 3), A.piece, ra, rb);
#pragma unroll
		for (int h = 0; h < 2; h++) {
			ia[h] = sa_pk_clamp(ia[h], ra, rb);
			ib[h] = sa_pk_clamp(ib[h], ra, rb);
		}
	}
	const int32_t chunk = t < nfull ? t - uload(A.tprefix + lo) : uload(A.tprefix + lo + 1) - uload(A.tprefix + lo);
	const int32_t ch_full = A.chunk;
	const int32_t i_begin = ra + chunk * (NGW * ch_full);
	const int32_t i_count = rb - i_begin < NGW * ch_full ? rb - i_begin : NGW * ch_full;
	/* a partial tile spreads its rows evenly over the row streams */
	const int32_t ch = (i_count + NGW - 1) / NGW;
	const int gw = wv * NG; /* this wave's first stream */
	/* Row store of this tile.  The rows of the matrix are cut into aligned blocks of A.lv[].rows sequences, and the
	 * ARRANGED copy of the store (sa_plan.cpp: sa_arrange_rows) holds every block's sequences in an order made for
	 * this tile shape: the k-th sequences of the streams of a wave have the same length wherever the block has enough
	 * sequences of that length.  Their terminators then pass at the same steps -- one event step serves all the groups
	 * of the wave -- and the streams end together (no bubbles).  A tile whose block lies inside the row range of its
	 * column pair streams positions [i_begin, i_begin + rows) of that copy; all tiles of the block do, so together
	 * they still cover the block's rows exactly once.  Scores find their rows through rowmap / posmap.
	 * Several block sizes are on offer (largest first): a tile takes the largest whose block fits -- every tile of that
	 * block then takes it too, a larger fitting block around one of them would be around all of them. */
	const uint8_t *rcodes = A.codes;
	const int32_t *roff = A.off, *rowmap = nullptr, *posmap = nullptr;
	int32_t sort_rows = 0;
	/* token streams of the level the tile streams (sa_plan.h: SaTokenStreams), or none: see the row streams below */
	const uint16_t *tk_tok = nullptr, *tk_mine = nullptr, *tk_any = nullptr;
	const int32_t *tk_off = nullptr;
	const uint32_t *tk_rows = nullptr; /* row streams of that level for this class's row stride (REGT below) */
	{
		const int32_t lvrows[SA_PK_SORT_LEVELS] = { uload(&A.lvp[0].rows), uload(&A.lvp[1].rows), uload(&A.lvp[2].rows),
							    uload(&A.lvp[3].rows) };
		static_assert(SA_PK_SORT_LEVELS == 4, "lvrows lists four levels");
		const int l = sa_pk_pick_level(lvrows, ra, rb, i_begin, NGW * ch_full);
		if (l >= 0) {
			const SaArranged &L = A.lvp[l];
			rcodes = uniform_ptr(L.codes);
			roff = uniform_ptr(L.off);
			rowmap = uniform_ptr(L.rowmap);
			posmap = uniform_ptr(L.posmap);
			tk_tok = uniform_ptr(L.tok);
			tk_off = uniform_ptr(L.tok_off);
			tk_mine = uniform_ptr(L.mine);
			tk_any = uniform_ptr(L.any);
			tk_rows = uniform_ptr(L.rowoff);
			sort_rows = lvrows[0]; /* (then the level's own, without a dynamic register index) */
#pragma unroll
			for (int k = 1; k < SA_PK_SORT_LEVELS; k++)
				if (l == k)
					sort_rows = lvrows[k];
		}
	}
	const bool sorted = sort_rows > 0;

	/* the substitution matrix, staged once per workgroup-tile in the storage the scores will use later */
	int8_t *const sub = reinterpret_cast<int8_t *>(s_out_all);
	for (int k = lane_id; k < SA_SUB_DIM * SA_SUB_DIM; k += 64 * WPB)
		sub[k] = A.sub8[k];
	/* ... and the residues of the two columns (padding: 0xff), in the ring storage -- coalesced loads, all in flight
	 * together; the build below read them from HBM one dependent byte load per column and lane (K round trips) */
	uint8_t *const s_cols = reinterpret_cast<uint8_t *>(s_ring_all);
	static_assert(2 * W <= WPB * NG * GSTRIDE * 2, "the staged columns fit the ring storage");
	for (int k = lane_id; k < 2 * W; k += 64 * WPB) {
		const int h = k >= W, c0 = k - h * W - pad[h];
		s_cols[k] = c0 >= 0 ? A.codes[offj[h] + c0] : (uint8_t)0xff;
	}
	__syncthreads();

	/* ---- query profile of the column pair: lanes holding the same columns split the table rows between them ---- */
	{
		constexpr int BUILDERS = NGW / COPIES; /* groups that hold a copy: they split its rows */
		constexpr int ROWS_EACH = (SA_CODE_ROWS + BUILDERS - 1) / BUILDERS;
		const int a_lo = ((gw + grp) / COPIES) * ROWS_EACH;
		uint8_t *const slot = s_prof + copy * (NSLOT * 16) + lig * 16;
		/* (unrolled a little -- the LDS round trips of four columns overlap -- but not fully: the build runs once per tile
		 * and must not set the kernel's register count) */
#pragma unroll 4
		for (int q = 0; q < K; q++) {
			int bq[2];
#pragma unroll
			for (int h = 0; h < 2; h++) {
				const int c = (int)s_cols[h * W + lig * K + q];
				bq[h] = c == 0xff ? -1 : c;
			}
#pragma unroll
			for (int r = 0; r < ROWS_EACH; r++) {
				const int a = a_lo + r;
				if (a >= SA_CODE_ROWS)
					break;
				uint32_t v = 0; /* SEP / NOP rows and padding columns: 0 (transparent, see header) */
#pragma unroll
				for (int h = 0; h < 2; h++) {
					int e = 0;
					if (a < SA_SUB_DIM && bq[h] >= 0) {
						e = (int)sub[a * SA_SUB_DIM + bq[h]] + A.pconst;
						/* Gotoh: the first real column sits right of a padding column whose N is one q too
						 * low: compensate in its diagonal term */
						if (METHOD == SA_METHOD_GA && pad[h] != 0 && lig * K + q == pad[h])
							e -= A.q;
					}
					v |= (uint32_t)(e & 0xffff) << (16 * h);
				}
				*reinterpret_cast<uint32_t *>(slot + a * ROWSTRIDE + (q >> 2) * PARTSTRIDE + (q & 3) * 4) = v;
			}
		}
	}

	/* ---- row streams: group g streams sequences [ib_g, ib_g + cnt_g) ---- */
	const int32_t ib_g = i_begin + (gw + grp) * ch;
	int32_t cnt_g = i_count - (gw + grp) * ch;
	cnt_g = cnt_g < 0 ? 0 : cnt_g > ch ? ch : cnt_g;
	const int32_t sbeg = roff[ib_g < A.num ? ib_g : 0];
	const int32_t slen = cnt_g > 0 ? roff[ib_g + cnt_g] - sbeg : 0;
	int32_t smax = 0; /* longest stream of the wave */
#pragma unroll
	for (int g = 0; g < NG; g++) {
		int32_t c = i_count - (gw + g) * ch;
		c = c < 0 ? 0 : c > ch ? ch : c;
		const int32_t b = i_begin + (gw + g) * ch;
		const int32_t l = c > 0 ? roff[b + c] - roff[b] : 0;
		smax = l > smax ? l : smax;
	}
	const int32_t steps = smax + G - 1;
	const int32_t nblk = (steps + 15) >> 4;
	const int32_t last = slen > 0 ? slen - 1 : 0;
	const int r16 = lane & 15;
	/* tokens a lane feeds per block: G = 8 two consecutive ones of its own group (positions 2k, 2k+1, k = r16 / 2),
	 * G = 16 the one at position r16 */
	constexpr int TPL = G == 8 ? 2 : 1;
	typedef typename std::conditional<G == 8, uint32_t, uint16_t>::type tok_t; /* ... as one LDS / global access */
	auto fpos = [&](int u) -> int { return G == 8 ? (r16 & ~1) + u : r16; };
	/* (32-bit offsets from the uniform base of the store: a scalar-base load, no 64-bit address arithmetic per token) */
	/* The three per-lane values the block work keeps across the main loop, one register each for BOTH ways to the tokens
	 * (below: the lean way): this one's are the offset of the lane's first position in the store, that of the stream's last
	 * position, and the stream's length.  (Separate variables per way are separate registers: the bundle kernels sit at
	 * their occupancy limits.) */
	uint32_t bw_a = (uint32_t)(sbeg + fpos(0)), bw_b = (uint32_t)(sbeg + last), bw_c = (uint32_t)slen;
	auto load_block = [&](int32_t blk, int u) -> int {
		const uint32_t at = bw_a + (uint32_t)u + (uint32_t)(blk << 4);
		return (int)rcodes[at < bw_b ? at : bw_b];
	};
	constexpr uint32_t SEPWORD = (uint32_t)SA_CODE_SEP * TUNIT;
	constexpr uint32_t NOPWORD = (uint32_t)SA_CODE_NOP * TUNIT;
	auto block_word = [&](int32_t blk, int raw, int u) -> uint32_t { /* token -> profile row offset */
		const int32_t pos = (blk << 4) + fpos(u);
		return pos < (int32_t)bw_c ? (uint32_t)raw * TUNIT : NOPWORD;
	};
	uint16_t *ring = s_ring + grp * GSTRIDE;
	auto ring_write = [&](int32_t blk, uint32_t word, int u) {
		const int i0 = ((blk << 4) + fpos(u)) & (RING - 1);
		ring[i0] = (uint16_t)word;
		ring[i0 + RING] = (uint16_t)word;
	};
	auto fold16 = [&](unsigned long long m) -> uint32_t {
		m |= m >> 32;
		m |= m >> 16;
		return (uint32_t)m & 0xffffu;
	};
	/* terminators of a block of tokens.  any: wave-uniform, bit p = some group's token at position p is a terminator;
	 * mine: this lane's group only (lanes 2k and 2k+1 of a DPP row hold positions 2k+u of their two groups) */
	auto block_events = [&](const uint32_t (&w)[TPL], uint32_t &mine) -> uint32_t {
		if (G == 16) {
			const unsigned long long m = __ballot(w[0] == SEPWORD);
			mine = (uint32_t)(m >> (lane & 48)) & 0xffffu;
			return fold16(m);
		}
		uint32_t any = 0;
		mine = 0;
#pragma unroll
		for (int u = 0; u < TPL; u++) {
			const unsigned long long m = __ballot(w[u] == SEPWORD);
			const uint32_t f = fold16(m);
			any |= ((f | (f >> 1)) & 0x5555u) << u;
			mine |= ((uint32_t)(m >> ((lane & 48) + (lane & 1))) & 0x5555u) << u;
		}
		return any;
	};

	/* The LEAN way to the same four things (next block's ring entries, gmask_next, evn, the prefetch for block + 2): a tile
	 * that streams an arranged level is a full tile whose streams are streams of the level's token copy (stream = position /
	 * chunk; host: sa_build_tokens) -- codes as u16 with NOP from the stream's end and padded past the lookahead, so a lane's
	 * two positions are ONE aligned dword at a constant offset from a base that moves 32 bytes per block (no clamp, no
	 * end-of-stream select), one multiply scales both, and the terminator masks are loaded instead of balloted.  One
	 * wave-uniform branch per block picks the way; the sixteen steps exist once. */
	/* (an integer in a scalar register: as a bool it lives in a lane mask and every block pays a v_cndmask + v_cmp to test it) */
	/* REGT: the lean way of this class takes its row offsets from the level's ROW STREAMS (sa_plan.h: sa_build_row_streams)
	 * straight into registers -- sixteen u32 byte offsets per lane and block, T(s) = that of stream position 16 blk + s - lig,
	 * four 16-byte loads at scalar base + constant lane offset, each issued into the registers of the quad the steps have
	 * just used up -- and the step's row address is lane_prof + T(s + 1).  No ring, no scaling, no per-step LDS read, and the
	 * terminator mask is ONE dword spanning the previous and the current block, so the event path tests constant bits.  The
	 * host builds the row streams of exactly these classes (sa_shapes.h: sa_pk_reg_tokens). */
	constexpr bool REGT = sa_pk_reg_tokens(METHOD, G, K);
	static_assert(!REGT || TSHIFT == 0, "a row stream holds byte offsets");
	const int32_t lean = __builtin_amdgcn_readfirstlane(tk_tok != nullptr && (!REGT || tk_rows != nullptr) ? 1 : 0);
	/* its three: bw_a = byte offset of this lane's tokens of block 0 in the token copy, bw_b = that of its stream's masks,
	 * bw_c = LDS byte offset at which it writes its tokens of a block 0 mod 4 (first ring copy) */
	const uint16_t *tk_any_w = nullptr;
	if (lean) {
		const int32_t s0 = i_begin / ch_full + gw; /* the wave's first stream (i_begin is a multiple of the chunk) */
		const uint32_t o_w = (uint32_t)uload(tk_off + s0), o_g = (uint32_t)tk_off[s0 + grp];
		bw_b = o_g >> 3; /* u16 per block: 2 (o_g / 16) bytes */
		tk_any_w = tk_any + (o_w >> 4) / NG;
		if (REGT) {
			/* byte offset of this lane's window of block 0 in the row streams: position -lig of its stream, which starts
			 * behind the front pads of the streams before it and its own (sa_plan.h: sa_row_stream_at) */
			bw_a = 4u * (o_g + (uint32_t)SA_ROW_FRONT * (uint32_t)(s0 + grp + 1) - (uint32_t)lig);
		} else {
			bw_a = 2u * o_g + (G == 8 ? 4u * (uint32_t)(r16 >> 1) : 2u * (uint32_t)r16);
			/* (with the offset of the rings folded in: derived from the ring READ base the write address is two instructions
			 * per block instead of one) */
			bw_c = (uint32_t)(WPB * OUT_HALFS * 2 + 2 * (wv * (NG * GSTRIDE) + grp * GSTRIDE + fpos(0)));
		}
	}
	/* The loads take the address form (uniform base in scalar registers + 32-bit lane offset): the base moves with the block
	 * in scalar arithmetic and the lane offset never changes.  The empty statement makes the offset a new value (in place)
	 * every block; loop-invariant, the compiler adds it to the base ONCE and then moves a 64-bit pointer per lane along
	 * (two registers and a 64-bit vector add per load). */
	auto lean_load = [&](int32_t blk) -> uint32_t {
		const uint8_t *const b = reinterpret_cast<const uint8_t *>(tk_tok) + (size_t)(uint32_t)(blk << 5);
		asm volatile("" : "+v"(bw_a));
		return *reinterpret_cast<const tok_t *>(b + bw_a);
	};
	auto lean_mine = [&](int32_t blk) -> uint32_t {
		const uint8_t *const b = reinterpret_cast<const uint8_t *>(tk_mine) + (size_t)(uint32_t)(blk << 1);
		asm volatile("" : "+v"(bw_b));
		return *reinterpret_cast<const uint16_t *>(b + bw_b);
	};
	/* REGT: quad qd = T(4 qd .. 4 qd + 3) of a block, one global_load_dwordx4 (the address is 4-byte aligned); the base moves
	 * 64 bytes per block in scalar arithmetic */
	typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
	typedef uint32_t u32_a2 __attribute__((aligned(2)));
	auto reg_load = [&](int32_t blk, int qd) -> u32x4 {
		const uint8_t *const b = reinterpret_cast<const uint8_t *>(tk_rows) + (size_t)(uint32_t)(blk << 6);
		asm volatile("" : "+v"(bw_a));
		return *reinterpret_cast<const u32x4_a4 *>(b + bw_a + 16 * qd);
	};
	/* ... and the stream's terminator masks of blocks blk - 1 (low half) and blk (high half) as one dword, blk >= 1 */
	auto reg_mine = [&](int32_t blk) -> uint32_t {
		const uint8_t *const b = reinterpret_cast<const uint8_t *>(tk_mine) + (size_t)(uint32_t)((blk << 1) - 2);
		asm volatile("" : "+v"(bw_b));
		return *reinterpret_cast<const u32_a2 *>(b + bw_b);
	};
	/* (every lane loads the wave's mask; it becomes scalar -- lean_any_s -- a block later: right behind the load the
	 * readfirstlane would wait for it) */
	auto lean_any = [&](int32_t blk) -> uint32_t { return (uint32_t)tk_any_w[blk]; };
	auto lean_any_s = [&](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
	/* REGT: the wave's mask of block blk >= 1 as the HIGH half of the dword that starts at block blk - 1 (no entry past the
	 * slot's last is read), made scalar and shifted down in scalar arithmetic: a u16 load that crosses a basic block costs a
	 * v_and for its upper half */
	auto reg_any = [&](int32_t blk) -> uint32_t { return *reinterpret_cast<const u32_a2 *>(tk_any_w + (blk - 1)); };
	auto reg_any_s = [&](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v) >> 16; };
	/* both tokens of the dword scaled at once: code < 64 and code * TUNIT < 65536, nothing carries into the upper half */
	auto lean_ring = [&](int32_t blk, uint32_t raw) {
		const uint32_t w = __umul24(raw, TUNIT);
		tok_t *const at = reinterpret_cast<tok_t *>(sa_pk_lds + bw_c + ((blk & 3) << 5));
		at[0] = (tok_t)w;
		at[RING * 2 / sizeof(tok_t)] = (tok_t)w;
	};

	/* ---- DP state (u16 pairs, see header) ---- */
	const uint32_t base2 = pk2((uint32_t)A.pk_base);
	const uint32_t delta2 = pk2((uint32_t)A.delta);
	const uint32_t q2 = pk2((uint32_t)-A.q); /* GA: |q| */
	const uint32_t cmask2 = (pad[0] == 0 ? 0xffffu : 0u) | (pad[1] == 0 ? 0xffff0000u : 0u); /* halves whose column 0 is real */
	uint32_t V[K], Y[K];
	uint32_t vl[2];   /* left-neighbour shift registers of even / odd steps (NW with paired adds: vl[0] alone, vl[1] is
	                   * never read); the first lane's copies hold what it injects */
	/* NW with paired adds keeps ONE left-neighbour register, vl[0] = X[0] of the header's X[K + 1]: the adds of a step run
	 * before its DPP move, when the register still holds the previous step's left value, and the move then overwrites it
	 * (the first lane has no source lane and keeps what it injects, which NW never changes).  X[] is not an array in the
	 * source: pkadd2's 64-bit operand (vl[0], V[0]) makes the register allocator put vl[0] in the even register below
	 * V[0], and (V[q - 1], V[q]) pins the rest of V[] pairwise.  Nothing but that operand constraint asks for it; what
	 * shows a compiler that builds the pairs with copies instead is the v_mov_b32 count of tools/dev/codegen_check.py
	 * (nw 8 9: no more of them than with SA_PK_PAIRED_ADDS=0). */
	constexpr bool PAIRED = SA_PK_PAIRED_ADDS && METHOD == SA_METHOD_NW;
	uint32_t xout = 0; /* GA: X of the column right of V[K-1], current row */
	uint32_t vbase;    /* GA: the plain boundary value (first lane) */
	/* SW (row-shifted domain of sa_systolic_kernel.inc: with p the stream position of the row a lane is processing it
	 * keeps V = No - (p+1)e and Y, X, M, floor, best each minus p*e; e < 0, so everything drifts UP by |e| per step --
	 * the drift of a whole tile is part of the range budget): */
	uint32_t fl = 0;             /* floor of the row this lane is processing (travels with the row)            */
	uint32_t flead = 0, xlead = 0; /* what the first lane starts a row with: the floor (= baseline) and the X boundary */
	uint32_t best = 0, carry = 0; /* running best of this lane's columns / of the row's sequence along the lanes  */
	const uint32_t e2 = pk2((uint32_t)-A.gap_e);             /* |e|      */
	const uint32_t gqs2 = pk2((uint32_t)(A.gap_e - A.gap_o)); /* |o - e|  */
	int32_t frame = 0; /* shifts of this group's frame so far */
	int nsep = 0;
	/* boundary value the first lane injects on an ordinary row: NW BASE, GA BASE + 2q; a terminator row injects
	 * cspecial more (GA: the corner, BASE + q) */
	const uint32_t inj0 = METHOD == SA_METHOD_NW ? base2 : base2 - 2 * q2;
	vl[0] = vl[1] = vbase = inj0;
	if (METHOD == SA_METHOD_SW) {
		/* a lane that starts at stream row -lig holds the top border as it looks in that row's domain */
		const uint32_t o2 = pk2((uint32_t)-A.gap_o);
		const uint32_t top = base2 - o2 - (uint32_t)lig * e2; /* BASE + o + lig e */
		vl[0] = base2 - o2 - e2; /* first lane only: o - (p+1)e after the -2e that precedes every use */
		vl[1] = top;
		xout = top - e2;
		xlead = base2 - o2;
		flead = base2;
		fl = base2 - (uint32_t)(lig + 1) * e2;
		best = base2 - (uint32_t)lig * e2;
#pragma unroll
		for (int q = 0; q < K; q++)
			V[q] = top, Y[q] = top;
	} else if (METHOD == SA_METHOD_NW) {
#pragma unroll
		for (int q = 0; q < K; q++)
			V[q] = base2, Y[q] = 0;
	} else {
		xout = base2 - q2; /* (the first lane's corner logic starts with the events of steps 0 and 1, see the event path) */
#pragma unroll
		for (int q = 0; q < K; q++)
			V[q] = inj0, Y[q] = inj0;
	}

	/* ---- prologue: empty ring, block 0 in the ring, block 1 in flight ---- */
	__syncthreads(); /* (every wave has read the staged columns out of the ring storage) */
	if (!(REGT && lean)) /* (the row-stream way has no ring; a tile that follows in this workgroup clears its own) */
		for (int k = lane; k < NG * GSTRIDE; k += 64)
			s_ring[k] = (uint16_t)NOPWORD;
	__syncthreads(); /* profile complete (all waves), ring cleared */
	/* Gotoh: the first sequence starts like after a terminator at stream position -1 */
	/* ev_hi: positions of the current block at which some group of the wave has a terminator (16 bits); ev_lo: the same
	 * for the previous block (all 32-bit scalar arithmetic: as 64-bit history the funnel shifts went through the VALU) */
	uint32_t ev_lo = METHOD == SA_METHOD_GA ? 0x8000u : 0u, ev_hi;
	/* gm: bit s + 2 = my group's token at position s of the current block is a terminator; bits 1, 0 = positions 15, 14
	 * of the previous block */
	/* REGT, lean: gm is the mask dword instead -- bit 16 + s = position s of the current block, bits 0..15 the previous block */
	uint32_t gm, gmask;
	u32x4 TQ[4] = {}; /* REGT, lean: T(s) = TQ[s >> 2][s & 3] */
	if (REGT && lean) {
#pragma unroll
		for (int qd = 0; qd < 4; qd++)
			TQ[qd] = reg_load(0, qd);
		gmask = lean_mine(0);
		ev_hi = lean_any_s(lean_any(0));
		gm = (gmask << 16) | (METHOD == SA_METHOD_GA ? 0x8000u : 0u);
	} else if (lean) {
		lean_ring(0, lean_load(0));
		gmask = lean_mine(0);
		ev_hi = lean_any_s(lean_any(0));
		gm = (gmask << 2) | (METHOD == SA_METHOD_GA ? 2u : 0u);
	} else {
		uint32_t w0[TPL];
#pragma unroll
		for (int u = 0; u < TPL; u++) {
			w0[u] = block_word(0, load_block(0, u), u);
			ring_write(0, w0[u], u);
		}
		ev_hi = block_events(w0, gmask);
		gm = (gmask << 2) | (METHOD == SA_METHOD_GA ? 2u : 0u);
	}
	/* What is in flight across a block.  The derived way: the code bytes of the block after the next.  The lean way:
	 * raw_next[0] = the lane's token dword of that block, mask_next = its stream's terminator mask and any_next the wave's,
	 * both of the NEXT block -- loaded a block before they are used, like the tokens.  With 8-lane groups mask_next IS
	 * raw_next[1]: both ways then load both registers in every block and the two unrolled blocks can swap them; a register
	 * that only one way loads costs that way a copy of the value just loaded, and a wait for it, where the ways join. */
	int raw_next[TPL];
	uint32_t mask_pf = 0, any_next = 0;
	uint32_t &mask_next = TPL == 2 ? reinterpret_cast<uint32_t &>(raw_next[TPL - 1]) : mask_pf;
	if (REGT && lean) {
		any_next = reg_any(1); /* (the stream's mask dword of a block is loaded in the block before it: do_block) */
	} else if (lean) {
		raw_next[0] = (int)lean_load(1);
		mask_next = lean_mine(1);
		any_next = lean_any(1);
	} else {
#pragma unroll
		for (int u = 0; u < TPL; u++)
			raw_next[u] = load_block(1, u);
	}
	const uint8_t *const lane_prof = s_prof + copy * (NSLOT * 16) + lig * 16;
	/* this lane's token of stream position 16 blk + s - lig sits at rbase[s] */
	auto ring_base = [&](int32_t blk) -> const uint16_t * { return ring + (((blk << 4) - lig) & (RING - 1)); };
	auto prof_row = [&](uint32_t word, uint4 (&P)[PARTS]) {
		const uint8_t *row = lane_prof + (word << TSHIFT);
#pragma unroll
		for (int p = 0; p < PARTS; p++)
			P[p] = *reinterpret_cast<const uint4 *>(row + p * PARTSTRIDE);
	};
	uint32_t tk_cur = 0, tk_nxt = 0;
	if (REGT && lean) {
		tk_cur = TQ[0][0];
	} else {
		const uint16_t *rb0 = ring_base(0);
		tk_cur = rb0[0], tk_nxt = rb0[1];
	}
	uint4 P[PARTS];
	prof_row(tk_cur, P);

	/* way: std::true_type = the row-stream way (REGT, lean tiles), std::false_type = the ring (lean or derived).  The steps
	 * exist once per way. */
	auto do_block = [&](auto way, const int32_t blk) __attribute__((always_inline)) {
		constexpr bool RW = decltype(way)::value;
		constexpr int MB = RW ? 16 : 2; /* bit of gm that stands for position 0 of the current block */
		if (A.rotate_prio) { /* (see the bundle kernel: fairness among the persistent waves of a SIMD) */
			switch (((uint32_t)A.rotate_prio + (uint32_t)blk) & 3u) {
			case 0: __builtin_amdgcn_s_setprio(0); break;
			case 1: __builtin_amdgcn_s_setprio(1); break;
			case 2: __builtin_amdgcn_s_setprio(2); break;
			default: __builtin_amdgcn_s_setprio(3); break;
			}
		}
		/* steps of this block at which a terminator enters the first lane of some group (+ Gotoh: the restore steps)
		 * or the last lane of some group meets one */
		const uint32_t ev_in =
			METHOD == SA_METHOD_GA ? (ev_hi | (ev_hi << 1) | (ev_hi << 2) | (ev_lo >> 15) | (ev_lo >> 14)) : ev_hi;
		const uint32_t ev = ((ev_lo >> (16 - (G - 1))) | (ev_hi << (G - 1)) | ev_in) & 0xffffu;
		/* next block's tokens go into the ring while this block computes */
		uint32_t gm_next = 0, evn; /* gm and ev_hi of the next block */
		/* (everything in flight was loaded a block ago and is used now: said once, here, the wait costs nothing, and the
		 * compiler's bookkeeping of the two ways' loads does not end in a wait for the NEW loads further down.  Not on the
		 * row-stream way: the quad loaded behind step 15 of the block before is still in flight and first read at step 11;
		 * the masks were loaded in front of it, and loads return in order) */
		if constexpr (!RW)
			__builtin_amdgcn_s_waitcnt(0x0f70); /* vmcnt(0) */
		if constexpr (RW) {
			/* (the next block's mask dword is in flight for this block only and becomes gm at its end: with a block of
			 * idling as gm_next, as on the ring way, three registers rotate through the two blocks of a trip and the back edge
			 * pays two copies) */
			evn = reg_any_s(any_next);
			asm volatile("" ::: "memory"); /* (what was in flight is consumed before its registers are loaded again) */
			mask_next = reg_mine(blk + 1);
			any_next = reg_any(blk + 2);
		} else if (!REGT && lean) { /* (REGT: the lean tiles of this class never come this way) */
			lean_ring(blk + 1, (uint32_t)raw_next[0]);
			gm_next = (mask_next << 2) | (gm >> 16);
			evn = lean_any_s(any_next);
			asm volatile("" ::: "memory"); /* (what was in flight is consumed before its registers are loaded again) */
			raw_next[0] = (int)lean_load(blk + 2);
			mask_next = lean_mine(blk + 2);
			any_next = lean_any(blk + 2);
		} else {
			uint32_t gmask_next;
			uint32_t wn[TPL];
#pragma unroll
			for (int u = 0; u < TPL; u++) {
				wn[u] = block_word(blk + 1, raw_next[u], u);
				ring_write(blk + 1, wn[u], u);
			}
			evn = block_events(wn, gmask_next);
			gm_next = (gmask_next << 2) | (gm >> 16);
#pragma unroll
			for (int u = 0; u < TPL; u++)
				raw_next[u] = load_block(blk + 2, u);
		}
		const uint16_t *rbase = RW ? nullptr : ring_base(blk);
		auto T = [&](int s) -> uint32_t { return TQ[(s >> 2) & 3][s & 3]; };

		/* One step of the block.  has_events = false is the same step without the event test: a block in which no
		 * terminator enters or leaves any group of the wave (ev == 0: ~70 % of the blocks of cfg 2) can run sixteen steps as ONE
		 * basic block -- no scalar bit test and branch per step, and the scheduler sees across the steps.  MEASURED AND
		 * SWITCHED OFF (SA_PK_QUIET_BLOCKS, round 4): the compiler's schedule of the merged block interleaves the adds of a
		 * step with the dependent maxima of the step before (s_nop 208 -> 38 per block) but holds more profile rows in
		 * flight -- 92 -> 128 VGPRs for NW K <= 16, 163 / 165 for Gotoh / SW (a wave per SIMD less) -- and doubles the loop's
		 * code: cfg 2 14.50 -> 15.18 ms, U[65,128] 33.3 -> 32.2 TCUPS.  The per-step branch costs nothing measurable. */
		auto step = [&](auto has_events, const int s) __attribute__((always_inline)) {
			uint32_t &vcur = vl[PAIRED ? 0 : s & 1];
			if (METHOD == SA_METHOD_SW)
				carry = pkmax(shift_in<G>(0u, carry), best);
			if (decltype(has_events)::value && __builtin_expect((ev >> s) & 1u, 0)) { /* wave-uniform, rare */
				/* the empty volatile statement keeps this a scalar branch (see sa_systolic_kernel.inc) */
				asm volatile("" ::: "memory");
				if ((gm >> (s + MB)) & 1u) { /* a terminator enters my group: shift the group's frame down by DELTA */
					/* One saturating subtraction per register (v_pk_sub_u16 clamp).  Whatever it clamps to 0 is stale
					 * -- at least PK_LIVE shifts old, see the header -- and has lost every max of a live row already.
					 * Only rows past the end of a stream (bubbles) can then see the Gotoh / SW subtractions wrap; their
					 * values travel with those rows and are never stored. */
#pragma unroll
					for (int q = 0; q < K; q++) {
						V[q] = pksubsat(V[q], delta2);
						if (METHOD != SA_METHOD_NW)
							Y[q] = pksubsat(Y[q], delta2);
					}
					if (METHOD != SA_METHOD_NW)
						xout = pksubsat(xout, delta2);
					if (METHOD == SA_METHOD_SW) { /* (xlead, flead and the first lane's vl[] are injections: not shifted) */
						fl = pksubsat(fl, delta2);
						best = pksubsat(best, delta2);
						carry = pksubsat(carry, delta2);
					}
					if (!leader) {
						vl[0] = pksubsat(vl[0], delta2);
						if (!PAIRED)
							vl[1] = pksubsat(vl[1], delta2);
					}
					frame++;
				}
				if (METHOD == SA_METHOD_GA && leader) {
					/* Terminator row t: the first lane injects the corner N[0][0] = BASE + q as the row's left value
					 * (it paints X' = q along the new top border).  Row t + 1: the diagonal input of column 0 is the
					 * corner only if column 0 is a real column; if it is padding the corner reaches the first real
					 * column through the padding (profile tweak) and column 0 must see the plain border -- a padding
					 * entry is 0 here, not the s32 kernels' -128, so it would not lose.  Row t + 2: plain again. */
					if ((gm >> (s + MB)) & 1u) {
						vl[(s + 1) & 1] = vbase;
						vcur = vbase + q2;
					} else if ((gm >> (s + MB - 1)) & 1u) {
						vl[(s + 1) & 1] = vbase + (q2 & cmask2);
					} else if ((gm >> (s + MB - 2)) & 1u) {
						vcur = vbase;
					}
				}
				if (lig == G - 1 && (RW ? T(s) : tk_cur) == SEPWORD) { /* a score pair leaves the pipeline */
					/* global: the sequence's last column; local: the best of all its cells, back from the row domain of
					 * its terminator row (that row's stream position times e) */
					const uint32_t v = METHOD == SA_METHOD_SW ? carry : V[K - 1];
					const int32_t rebase = (frame - nsep) * A.delta - A.pk_base + /* back into this sequence's own frame */
							       (METHOD == SA_METHOD_SW ? ((blk << 4) + s - (G - 1)) * A.gap_e : 0);
					s_out[grp * CH + nsep] = (int16_t)((int32_t)(v & 0xffffu) + rebase);
					s_out[NG * CH + grp * CH + nsep] = (int16_t)((int32_t)(v >> 16) + rebase);
					nsep++;
				}
			}
			/* token two steps ahead (positions 16, 17 belong to the next block, already in the ring).  Loaded BEHIND the event
			 * branch: load and the step's end then sit in one basic block (see SA_PK_OPAQUE_TOKEN below) */
			uint32_t tk_far = 0;
			if constexpr (!RW)
				tk_far = rbase[s + 2];
			const uint32_t vprev = vl[PAIRED ? 0 : (s + 1) & 1];
			/* Diagonal adds are made just in time (column q + 1's from the still-old V[q]), and a 16-byte part of the
			 * profile row is re-loaded for the NEXT step as soon as its four columns have been consumed -- no d[] array,
			 * no second profile buffer.  A packed op that reads the result of the packed op right before it costs a
			 * wait state, so independent work of the next columns sits between the dependent ops of the chain. */
			/* (the row-stream way: step 15 reads the next block's T(0), loaded into quad 0 behind step 3) */
			const uint8_t *const row_next = lane_prof + (RW ? T(s + 1) : tk_nxt << TSHIFT);
			auto reload = [&](int q_done) { /* columns 0..q_done are consumed */
				if ((q_done & 3) == 3 || q_done == K - 1) {
					P[q_done >> 2] = *reinterpret_cast<const uint4 *>(row_next + (q_done >> 2) * PARTSTRIDE);
					/* a partly used last part stays ONE ds_read_b128 (the empty statement "uses" the tail): narrowed to
					 * b32 / b64 / b96 it is served in wider lane phases whose lanes share bank windows */
					if ((K & 3) != 0 && (q_done >> 2) == PARTS - 1)
						asm volatile("" ::"v"(P[PARTS - 1].y), "v"(P[PARTS - 1].z), "v"(P[PARTS - 1].w));
				}
			};
			uint32_t dnw[K];
			if (METHOD == SA_METHOD_NW) {
				if (PAIRED) {
					/* columns q, q + 1 for even q: (X[q], X[q + 1]) + (S'[q], S'[q + 1]), the profile pair being components
					 * 0/1 or 2/3 of a ds_read_b128; odd K keeps a plain add for its last column */
#pragma unroll
					for (int q = 0; q + 1 < K; q += 2)
						pkadd2(q ? V[q - 1] : vprev, V[q], comp(P[q >> 2], q & 3), comp(P[q >> 2], (q & 3) + 1), dnw[q], dnw[q + 1]);
					if (K & 1)
						dnw[K - 1] = (K > 1 ? V[K > 1 ? K - 2 : 0] : vprev) + comp(P[(K - 1) >> 2], (K - 1) & 3);
				} else {
					dnw[0] = vprev + comp(P[0], 0);
#pragma unroll
					for (int q = 1; q < K; q++)
						dnw[q] = V[q - 1] + comp(P[q >> 2], q & 3);
				}
#pragma unroll
				for (int p = 0; p < PARTS; p++) /* the profile row of the next step, into the registers the adds released */
					P[p] = *reinterpret_cast<const uint4 *>(row_next + p * PARTSTRIDE);
				if ((K & 3) != 0) { /* (keeps the partly used last part one ds_read_b128, see reload) */
					if (PAIRED) /* (as ONE operand: with a 64-bit use beside 32-bit ones the load is split into a ds_read2_b64) */
						asm volatile("" ::"v"(__builtin_bit_cast(u32x4, P[PARTS - 1])));
					else
						asm volatile("" ::"v"(P[PARTS - 1].y), "v"(P[PARTS - 1].z), "v"(P[PARTS - 1].w));
				}
				__builtin_amdgcn_sched_barrier(0);
			}
			if (METHOD == SA_METHOD_SW)
				vcur += 2 * e2; /* the first lane's boundary values follow the stream position of its row */
			const uint32_t vleft = vcur = shift_in<G>(vcur, V[K - 1]);
			if (METHOD == SA_METHOD_SW) {
				uint32_t x = shift_in<G>(xlead, xout);
				fl = shift_in<G>(flead, fl); /* the first lane: the current baseline */
				xlead += e2;
				flead += e2;
				if (F16) {
					/* y = max3(V, Y, floor); m = max3(d, y, x); the running best takes two columns per op */
					uint32_t d = vprev + comp(P[0], 0), mprev = 0;
#pragma unroll
					for (int q = 0; q < K; q++) {
						const uint32_t y = pkmax3<true>(V[q], Y[q], fl);
						Y[q] = y;
						uint32_t dn = 0;
						if (q + 1 < K) {
							dn = V[q] + comp(P[(q + 1) >> 2], (q + 1) & 3);
							reload(q + 1);
						} else if (K == 1) {
							reload(0);
						}
						const uint32_t m = pkmax3<true>(d, y, x);
						if (q & 1)
							best = pkmax3<true>(best, mprev, m);
						else if (q == K - 1)
							best = pkmax(best, m);
						mprev = m;
						V[q] = m - gqs2;
						x = pkmax(V[q], x) - e2;
						d = dn;
					}
				} else {
					uint32_t t0;
					{
						const uint32_t y = pkmax(pkmax(V[0], Y[0]), fl);
						Y[0] = y;
						t0 = pkmax(vprev + comp(P[0], 0), y);
						if (K == 1)
							reload(0);
					}
#pragma unroll
					for (int q = 0; q < K; q++) {
						/* the floor is applied to Y instead of M: M = max(d, X, Y) >= Y >= floor, and a floored Y only
						 * adds candidates <= floor + e to later cells, which cannot change any M (sa_systolic_kernel.inc) */
						const uint32_t m = pkmax(t0, x);
						if (q + 1 < K) {
							const uint32_t y = pkmax(pkmax(V[q + 1], Y[q + 1]), fl);
							Y[q + 1] = y;
							t0 = pkmax(V[q] + comp(P[(q + 1) >> 2], (q + 1) & 3), y);
							reload(q + 1);
						}
						best = pkmax(best, m);
						V[q] = m - gqs2;
						x = pkmax(V[q], x) - e2;
					}
				}
				best += e2; /* into the next row's domain */
				xout = x;
			} else if (METHOD == SA_METHOD_NW) {
				/* (NW keeps its K diagonal adds ahead of the chain -- issued before the DPP move, above: measured 2.6 %
				 * faster than just-in-time adds) */
				if (F16) {
#if SA_PK_CHAINED_MAX3
					pkmax3_chain_all<K>(V, dnw, vleft);
#else
#pragma unroll
					for (int q = 0; q < K; q++)
						V[q] = pkmax3<true>(dnw[q], V[q], q ? V[q - 1] : vleft);
#endif
				} else {
					uint32_t tq[K];
					tq[0] = pkmax(dnw[0], V[0]);
					if constexpr (K > 1)
						tq[1] = pkmax(dnw[1], V[1]);
#pragma unroll
					for (int q = 0; q < K; q++) {
						V[q] = pkmax(tq[q], q ? V[q - 1] : vleft);
						if (q + 2 < K)
							tq[q + 2] = pkmax(dnw[q + 2], V[q + 2]);
					}
				}
			} else {
				uint32_t x = shift_in<G>(vleft, xout);
				if (F16) {
					uint32_t d = vprev + comp(P[0], 0);
#pragma unroll
					for (int q = 0; q < K; q++) {
						const uint32_t y = pkmax(V[q], Y[q]);
						Y[q] = y;
						uint32_t dn = 0;
						if (q + 1 < K) {
							dn = V[q] + comp(P[(q + 1) >> 2], (q + 1) & 3);
							reload(q + 1);
						} else if (K == 1) {
							reload(0);
						}
						const uint32_t m = pkmax3<true>(d, y, x);
						V[q] = m - q2;
						x = pkmax(V[q], x);
						d = dn;
					}
				} else {
					uint32_t t0;
					{
						const uint32_t y = pkmax(V[0], Y[0]);
						Y[0] = y;
						t0 = pkmax(vprev + comp(P[0], 0), y);
						if (K == 1)
							reload(0);
					}
#pragma unroll
					for (int q = 0; q < K; q++) {
						const uint32_t m = pkmax(t0, x);
						if (q + 1 < K) {
							const uint32_t y = pkmax(V[q + 1], Y[q + 1]);
							Y[q + 1] = y;
							t0 = pkmax(V[q] + comp(P[(q + 1) >> 2], (q + 1) & 3), y);
							reload(q + 1);
						}
						V[q] = m - q2;
						x = pkmax(V[q], x);
					}
				}
				xout = x;
			}
			if constexpr (RW) {
				/* the quad whose last offset was this step's own is used up: the next block's, into the same registers */
				if ((s & 3) == 3)
					TQ[s >> 2] = reg_load(blk + 1, s >> 2);
			} else {
			tk_cur = tk_nxt;
#if SA_PK_OPAQUE_TOKEN
			/* The token travels through the loop as a 32-bit value the optimiser cannot narrow back to the u16 it was loaded
			 * as: a loop-carried u16 has no defined upper half, and its use as an address offset became v_add_u32_sdwa
			 * (WORD_0 select: an SDWA instruction, ~4.1 issue cycles) where a plain v_add_u32 (~2.5) does.  Instruction
			 * selection works per basic block and the event branch splits the steps, so the zero extension of the load is
			 * only known to be free where load and use share a block: the load sits behind the event branch and the empty
			 * statement at the END of the same step, where the load (the step's last LDS operation) has to have landed for
			 * the next step's profile reads anyway -- right behind the load it would put a wait in front of every step. */
			uint32_t tk_wide = tk_far;
			asm volatile("" : "+v"(tk_wide));
			tk_nxt = tk_wide;
#else
			tk_nxt = tk_far;
#endif
			}
		};
		/* (where the registers allow it: the quiet block's schedule holds more rows of the profile in flight -- NW, K <= 16:
		 * 92 -> 128 VGPRs, still four waves per SIMD; NW K = 17..24 would go 119 -> 167, Gotoh / SW K = 9..16 to 163 / 165:
		 * a wave per SIMD less, so those keep the stepwise form) */
		constexpr bool QUIET = SA_PK_QUIET_BLOCKS && METHOD == SA_METHOD_NW && G == 8 && K <= 16;
		if (QUIET && ev == 0) {
#pragma unroll
			for (int s = 0; s < 16; s++)
				step(std::false_type{}, s);
		} else {
#pragma unroll
			for (int s = 0; s < 16; s++)
				step(std::true_type{}, s);
		}
		if constexpr (RW)
			gm = mask_next;
		else
			gm = gm_next;
		ev_lo = ev_hi;
		ev_hi = evn;
	};
	const unsigned long long ph1 = A.stamps ? __builtin_amdgcn_s_memtime() : 0ull; /* diagnostics: end of the prologue */
	/* two blocks per trip: the compiler leaves a register copy per loop-carried DP value on the back edge */
	if (REGT && lean) {
		if constexpr (REGT)
			for (int32_t blk2 = 0; blk2 < nblk; blk2 += 2) {
				do_block(std::true_type{}, blk2);
				if (blk2 + 1 < nblk)
					do_block(std::true_type{}, blk2 + 1);
			}
	} else {
		for (int32_t blk2 = 0; blk2 < nblk; blk2 += 2) {
			do_block(std::false_type{}, blk2);
			if (blk2 + 1 < nblk)
				do_block(std::false_type{}, blk2 + 1);
		}
	}
	if (A.stamps && threadIdx.x == 0) { /* diagnostics: shader clock at the end of the prologue and of the main loop, steps */
		A.stamps[3 * (size_t)A.nlocal + 3 * (size_t)A.stamp_u + 0] = ph1;
		A.stamps[3 * (size_t)A.nlocal + 3 * (size_t)A.stamp_u + 1] = __builtin_amdgcn_s_memtime();
		A.stamps[3 * (size_t)A.nlocal + 3 * (size_t)A.stamp_u + 2] = (unsigned long long)nblk * 16;
	}
	__syncthreads();

	/* ---- epilogue: un-bias and store ---- */
	if (A.dense_off) {
		/* dense share (tile-interleaved sharding): the scores of the tile's row streams leave in POSITION order, one
		 * run per column -- no rowmap, no range test; sa_k_place maps positions to rows after the all-gather */
		const int64_t draw = A.dense_off[t];
		const int64_t dbase = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(draw >> 32)) << 32) |
						(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)draw));
		const int32_t cntp = SA_SHARE_PAD(i_count);
#pragma unroll
		for (int g = 0; g < NG; g++) {
			int32_t c = i_count - (gw + g) * ch;
			c = c < 0 ? 0 : c > ch ? ch : c;
			if (lane < c && active) {
				const int32_t is = i_begin + (gw + g) * ch + lane;
				const int32_t m = roff[is + 1] - roff[is] - 1;
#pragma unroll
				for (int h = 0; h < 2; h++) {
					if (h == 1 && dup)
						continue;
					const int32_t raw = s_out[h * NG * CH + g * CH + lane];
					int32_t score;
					if (METHOD == SA_METHOD_NW)
						score = raw + (m + nh[h]) * A.gap_g;
					else if (METHOD == SA_METHOD_GA)
						score = raw - A.q + (m + nh[h]) * A.gap_e;
					else
						score = raw;
					const int64_t at = dbase + h * cntp + (is - i_begin);
					if (A.out16)
						reinterpret_cast<int16_t *>(A.out)[at] = (int16_t)score;
					else
						A.out[at] = score;
				}
			}
		}
		if (!A.host_out)
			return;
		/* ... and, with a page-locked host matrix to deliver to, the same scores once more in the reference's packed order,
		 * straight into it (below): the host copy of a multi-GPU run costs no copy pass and waits for no gather */
	}
	/* destination of the packed-order stores: the launch's output, or the host matrix next to a dense share */
	int32_t *const pout = A.dense_off ? A.host_out : A.out;
	const bool p16 = A.dense_off ? false : A.out16 != 0;
	const bool pnt = A.dense_off ? true : A.out_nt != 0;
	if (sorted && sort_rows == NGW * ch_full) {
		/* The tile is the whole block: its scores leave in row order.  Every wave stores one contiguous quarter of the
		 * tile's rows, a lane four consecutive rows per round -- one 16-byte (int16 scores: 8-byte) store per lane and
		 * column, 1 KB per wave instruction, where all four rows belong to the column's range. */
		if (active) {
			constexpr int E = 4;
			const int32_t wrows = NG * ch_full; /* (a multiple of 4) */
			for (int32_t n = 0; n < wrows; n += 64 * E) {
				const int32_t r0 = n + E * lane;
				if (r0 >= wrows)
					continue;
				const int32_t i0 = i_begin + wv * wrows + r0;
				int32_t sc[2][E];
#pragma unroll
				for (int e = 0; e < E; e++) {
					const int32_t i = i0 + e;
					const int32_t p = posmap[i] - i_begin; /* position in the tile: stream * chunk + sequence */
					const int32_t st = p / ch_full, k = p - st * ch_full;
					const int16_t *const so = s_out_all + (st / NG) * OUT_HALFS + (st % NG) * CH + k;
					const int32_t m = A.off[i + 1] - A.off[i] - 1;
#pragma unroll
					for (int h = 0; h < 2; h++) {
						const int32_t raw = so[h * NG * CH];
						if (METHOD == SA_METHOD_NW)
							sc[h][e] = raw + (m + nh[h]) * A.gap_g;
						else if (METHOD == SA_METHOD_GA)
							sc[h][e] = raw - A.q + (m + nh[h]) * A.gap_e;
						else
							sc[h][e] = raw;
					}
				}
#pragma unroll
				for (int h = 0; h < 2; h++) {
					if (h == 1 && dup)
						continue;
					const int64_t at = tri[h] + i0 - A.start;
					if (i0 >= ia[h] && i0 + E <= ib[h]) {
						typedef int32_t i32x4 __attribute__((ext_vector_type(4), aligned(4)));
						typedef int16_t i16x4 __attribute__((ext_vector_type(4), aligned(2)));
						if (p16) {
							i16x4 v = { (int16_t)sc[h][0], (int16_t)sc[h][1], (int16_t)sc[h][2], (int16_t)sc[h][3] };
							SA_PK_STORE(pnt, v, reinterpret_cast<i16x4 *>(reinterpret_cast<int16_t *>(pout) + at));
						} else {
							i32x4 v = { sc[h][0], sc[h][1], sc[h][2], sc[h][3] };
							SA_PK_STORE(pnt, v, reinterpret_cast<i32x4 *>(pout + at));
						}
						continue;
					}
#pragma unroll
					for (int e = 0; e < E; e++) { /* a column whose range ends inside these four rows */
						const int32_t i = i0 + e;
						if (i < ia[h] || i >= ib[h])
							continue;
						if (p16)
							SA_PK_STORE(pnt, (int16_t)sc[h][e], &reinterpret_cast<int16_t *>(pout)[at + e]);
						else
							SA_PK_STORE(pnt, sc[h][e], &pout[at + e]);
					}
				}
			}
		}
		return;
	}
#pragma unroll
	for (int g = 0; g < NG; g++) {
		int32_t c = i_count - (gw + g) * ch;
		c = c < 0 ? 0 : c > ch ? ch : c;
		if (lane < c && active) {
			const int32_t is = i_begin + (gw + g) * ch + lane; /* position in the row store of this tile */
			const int32_t i = sorted ? rowmap[is] : is;     /* the row it is                        */
			const int32_t m = roff[is + 1] - roff[is] - 1;
#pragma unroll
			for (int h = 0; h < 2; h++) {
				if (i < ia[h] || i >= ib[h] || (h == 1 && dup))
					continue;
				const int32_t raw = s_out[h * NG * CH + g * CH + lane];
				int32_t score;
				if (METHOD == SA_METHOD_NW)
					score = raw + (m + nh[h]) * A.gap_g;
				else if (METHOD == SA_METHOD_GA)
					score = raw - A.q + (m + nh[h]) * A.gap_e;
				else
					score = raw;
				if (p16)
					SA_PK_STORE(pnt, (int16_t)score, &reinterpret_cast<int16_t *>(pout)[tri[h] + i - A.start]);
				else
					SA_PK_STORE(pnt, score, &pout[tri[h] + i - A.start]);
			}
		}
	}
}

/* (an occupancy floor -- amdgpu_waves_per_eu 4 for NW, 3 for Gotoh / SW, i.e. <= 128 / 168 VGPRs -- was measured: no gain,
 * the kernels are bound by VALU issue, not by latency) */
/* One persistent launch for up to SA_PK_BUNDLE classes K = KLO .. KLO + 7 (sa_internal.h: SaPkClassArgs): workgroups
 * pull the launch's tiles from a device counter in the order of A0.ulist -- the full tiles class after class (largest K
 * first), then the partial tiles of all classes by decreasing size. */
template <int METHOD, int G, int KLO, bool F16>
__global__ __launch_bounds__(64 * sa_pk_wpb(METHOD, G, KLO)) void sa_k_systolic_pk_bundle(SaSysArgs A0)
{
	__shared__ int32_t s_next;
	constexpr int KMAX = G == 8 ? SA_PK_KMAX : SA_PK16_KMAX;
	/* Stagger.  The workgroups of a launch start together and, their tiles being of equal size, stay in step: every
	 * workgroup of a SIMD would be in its latency-bound prologue / epilogue (global loads, barriers: ~35 000 clocks per
	 * tile) at the same time, with no other wave's arithmetic to hide it behind -- a tenth of a 256-row tile, and a short
	 * launch (one rank's share of a multi-GPU run) never drifts out of step.  So the workgroup in wave slot s of its SIMD
	 * starts s * A0.stagger sleep periods late: the four workgroups that share a SIMD then take turns. */
	if (A0.stagger > 0) {
		if (threadIdx.x == 0)
			s_next = (int32_t)(__builtin_amdgcn_s_getreg((3 << 11) | 4) & 3u); /* HW_ID.wave_id: this wave's slot on its SIMD */
		__syncthreads();
		const int32_t n = __builtin_amdgcn_readfirstlane(s_next) * A0.stagger;
		for (int32_t k = 0; k < n; k++)
			__builtin_amdgcn_s_sleep(127);
		__syncthreads();
	}
	/* Rotating wave priority.  The issue arbiter serves the oldest wave of a SIMD first, and in these ALU-bound loops three
	 * waves saturate it (Gotoh, SW): the youngest of the four persistent workgroups of a CU starved for the WHOLE launch --
	 * SA_HIP_STAMPS showed 256 workgroups (one per CU) spending 98 % of a share's launch on their first tile and finishing
	 * it alone at the end, a tail of 7 %.  So every wave takes the priority (its hardware wave slot + block number) mod 4,
	 * anew every 16 steps (pk_tile: do_block): the four waves of a SIMD differ while they run in step, the favoured one
	 * changes 50 times per tile, and all of them advance at the same average rate.  (Rotating per TILE only moved the
	 * starvation around: strict priorities are as unfair as age.) */
	const uint32_t wave_slot = __builtin_amdgcn_s_getreg((3 << 11) | 4); /* HW_ID.wave_id */
	for (;;) {
		if (threadIdx.x == 0)
			s_next = (int32_t)atomicAdd(A0.counter, 1u);
		__syncthreads();
		const int32_t u = __builtin_amdgcn_readfirstlane(s_next);
		__syncthreads();
		if (u >= A0.nlocal)
			break;
		const uint32_t ut = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)A0.ulist[2 * (size_t)u]);
		const int c = (int)(ut >> SA_PK_UTILE_BITS);
		const int32_t t = (int32_t)(ut & ((1u << SA_PK_UTILE_BITS) - 1u));
		/* The class block lives in global memory, which this kernel also writes: the compiler cannot prove these loads
		 * unclobbered, issues them as vector loads and would keep the whole tile geometry derived from them in VGPRs
		 * (+50).  They are wave-uniform: say so. */
		const SaPkClassArgs &P = A0.pkc[c];
		SaSysArgs A = A0;
		A.tile_pair = __builtin_amdgcn_readfirstlane((int32_t)A0.ulist[2 * (size_t)u + 1]);
		A.jlist = uniform_ptr(P.jlist);
		A.tprefix = uniform_ptr(P.tprefix);
		A.dense_off = uniform_ptr(P.dense_off);
		A.ncols = __builtin_amdgcn_readfirstlane(P.ncols);
		A.npart = __builtin_amdgcn_readfirstlane(P.npart);
		A.delta = __builtin_amdgcn_readfirstlane(P.delta);
		A.pk_base = __builtin_amdgcn_readfirstlane(P.pk_base);
		A.rotate_prio = A0.rotate_prio ? (int32_t)(4u + (wave_slot & 3u)) : 0;
		A.chunk = __builtin_amdgcn_readfirstlane(P.chunk);
		A.piece = __builtin_amdgcn_readfirstlane(P.piece);
		A.lvp = P.lv; /* (the tile reads the one arranged copy it streams from there: 20 fewer live SGPRs) */
		const int32_t ntiles = __builtin_amdgcn_readfirstlane(A.tprefix[(A.ncols + 1) >> 1]) + A.npart;
		const unsigned long long st0 = A0.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
		const unsigned long long sc0 = A0.stamps ? __builtin_amdgcn_s_memtime() : 0ull;
		A.stamp_u = u;
		switch (__builtin_amdgcn_readfirstlane(P.k) - KLO) {
#define SA_BCASE(D)                                                  \
	case D:                                                      \
		if constexpr (KLO + D <= KMAX)                       \
			pk_tile<METHOD, G, KLO + D, F16>(A, t, ntiles); \
		break;
			SA_BCASE(0) SA_BCASE(1) SA_BCASE(2) SA_BCASE(3) SA_BCASE(4) SA_BCASE(5) SA_BCASE(6) SA_BCASE(7)
#undef SA_BCASE
		default:
			break;
		}
		/* (the barrier at the top of the loop separates this tile's epilogue reads from the next tile's LDS writes) */
		if (A0.stamps && threadIdx.x == 0) { /* diagnostics (SA_HIP_STAMPS): when this workgroup ran launch-tile u, 100 MHz ticks */
			A0.stamps[3 * (size_t)u + 0] = st0;
			A0.stamps[3 * (size_t)u + 1] = __builtin_amdgcn_s_memrealtime();
			A0.stamps[3 * (size_t)u + 2] = sc0; /* shader clock at the start of the tile */
			A0.stamps[6 * (size_t)A0.nlocal + (size_t)u] = __builtin_amdgcn_s_memtime();
		}
	}
	/* The last workgroup to leave puts the counters back to zero for the next launch that uses them: no memset (a fill
	 * kernel and a barrier, ~30 us) in front of every launch.  Every workgroup has made its last fetch before it counts
	 * itself out, so the reset cannot race with a fetch. */
	if (threadIdx.x == 0) {
		__threadfence();
		if (atomicAdd(A0.counter + 1, 1u) == gridDim.x - 1) {
			atomicExch(A0.counter, 0u);
			atomicExch(A0.counter + 1, 0u);
		}
	}
}

template <int METHOD, int G, int KLO, bool F16>
hipError_t launch_bundle(const SaSysArgs &a, int wgs, unsigned lds_bytes, hipStream_t s)
{
	auto *kern = &sa_k_systolic_pk_bundle<METHOD, G, KLO, F16>;
	if (lds_bytes > 64 * 1024) { /* (K >= 37 with 16-lane groups: opt in to more than 64 KB of dynamic LDS, once per kernel and device) */
		static std::atomic<unsigned long long> raised{ 0 }; /* bit d: done on device d */
		int dev = 0;
		(void)hipGetDevice(&dev);
		const unsigned long long bit = 1ull << (dev & 63);
		if (!(raised.load() & bit)) {
			(void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
						  sa_pk_lds_bytes(METHOD, G, KLO + SA_PK_BUNDLE - 1 < (G == 8 ? SA_PK_KMAX : SA_PK16_KMAX) ? KLO + SA_PK_BUNDLE - 1
														   : (G == 8 ? SA_PK_KMAX : SA_PK16_KMAX)));
			(void)hipGetLastError();
			raised.fetch_or(bit);
		}
	}
	static_assert(sa_pk_wpb(METHOD, G, KLO) == sa_pk_wpb(METHOD, G, KLO + SA_PK_BUNDLE - 1), "a bundle does not straddle the workgroup sizes");
	hipLaunchKernelGGL(kern, dim3(wgs), dim3(64 * sa_pk_wpb(METHOD, G, KLO)), lds_bytes, s, a);
	return hipGetLastError();
}

template <int METHOD> hipError_t launch_pk(int g, int klo, int f16, const SaSysArgs &a, int wgs, unsigned lds_bytes, hipStream_t s)
{
	/* (one translation unit = one code object per method and group width: a store of short sequences never loads the
	 * 16-lane kernels, two thirds of the packed code) */
	if (g != SA_PK_G || !a.pkc || a.npkc < 1 || a.npkc > 2 * SA_PK_VARIANTS * SA_PK_BUNDLE) /* (every class once per tile size and variant) */
		return hipErrorInvalidValue;
#if SA_PK_G == 8
	if (!f16)
		return hipErrorInvalidValue;
	switch (klo) {
	case 1:
		return launch_bundle<METHOD, 8, 1, true>(a, wgs, lds_bytes, s);
	case 9:
		return launch_bundle<METHOD, 8, 9, true>(a, wgs, lds_bytes, s);
	case 17:
		return launch_bundle<METHOD, 8, 17, true>(a, wgs, lds_bytes, s);
	default:
		return hipErrorInvalidValue;
	}
#else
#define SA_B16(KLO_)                                                                        \
	case KLO_:                                                                          \
		return f16 ? launch_bundle<METHOD, 16, KLO_, true>(a, wgs, lds_bytes, s)    \
			   : launch_bundle<METHOD, 16, KLO_, false>(a, wgs, lds_bytes, s);
	/* (the 16-lane bundles of a method are two translation units -- K up to 44, K from 45 -- so that they compile side
	 * by side: each is minutes of compile time) */
	switch (klo) {
#if SA_PK16_PART == 0
		SA_B16(13) SA_B16(21) SA_B16(29) SA_B16(37)
#else
		SA_B16(45)
	case 53: /* (past SA_PK16_F16_KMAX: the two-way form only) */
		return f16 ? hipErrorInvalidValue : launch_bundle<METHOD, 16, 53, false>(a, wgs, lds_bytes, s);
	case 61:
		return f16 ? hipErrorInvalidValue : launch_bundle<METHOD, 16, 61, false>(a, wgs, lds_bytes, s);
#endif
	default:
		return hipErrorInvalidValue;
	}
#undef SA_B16
#endif
}

} // namespace

hipError_t SA_SYS_LAUNCH(int g, int klo, int f16, const SaSysArgs &a, int wgs, unsigned lds_bytes, hipStream_t s)
{
	return launch_pk<SA_SYS_METHOD>(g, klo, f16, a, wgs, lds_bytes, s);
}

hipError_t SA_SYS_WARM(void)
{
	hipFuncAttributes attr;
#if SA_PK_G == 8
	return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sa_k_systolic_pk_bundle<SA_SYS_METHOD, 8, 9, true>));
#else
#if SA_PK16_PART == 0
	return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sa_k_systolic_pk_bundle<SA_SYS_METHOD, 16, SA_PK_K16_MIN, true>));
#else
	return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sa_k_systolic_pk_bundle<SA_SYS_METHOD, 16, 45, false>));
#endif
#endif
}
