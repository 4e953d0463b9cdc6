/*
 * sa_traceback.hip -- alignments for chosen pairs: the decisions of every DP cell recorded on the device, walked back and
 * returned as run-length CIGARs (sa_ctx_alignments, sa_hip_alignments).  No reference counterpart: the reference keeps
 * scores only.  The contract -- orientation, tie rule, what a CIGAR scores -- is in include/seqalign_hip.h; the record of a
 * cell, the scratch layout and one step of the walk are in sa_traceback_core.h, which the host compiles as well.
 *
 *   sa_k_trace_fill<METHOD>  one pair per wavefront: the sweep of sa_k_pair_per_wave (sa_generic.hip) restated -- lane l owns
 *                            column 64 s + l + 1, rows travel one lane per step, the strip's last column is parked in the
 *                            context's boundary scratch -- plus one record byte per cell.  A lane packs four steps into a
 *                            word, so a wave stores 256 contiguous bytes every fourth step.  SW also keeps its end cell under
 *                            the key (best descending, r ascending, c ascending), per lane first, then over the wave.
 *   sa_k_trace_walk<METHOD>  one pair per wavefront, wave-uniform: follows the records from the end cell.  A walk is a chain of
 *                            dependent loads; the records a step can reach lie at most 257 bytes below the current one, so the
 *                            wave fetches the kilobyte that ends at the current record in one load per lane, parks it in LDS
 *                            and takes the next eight to sixteen steps from there.  Runs are written end-first, downwards
 *                            from the end of the pair's area of m + n words.
 *   FIT = true               the fit contract (sa_fit_core.h; sa_ctx_fit_alignments): the fill feeds M[r][0] = 0 in lane 0 of strip 0
 *                            and the lane that owns column n keeps the end cell (M descending, r ascending, row 0 included); the walk
 *                            takes its steps through sa_tb_step_fit.  Everything else is the one body.
 *   sa_k_trace_scan          exclusive scan of cigar_len in the caller's pair order -> cigar_off
 *   sa_k_trace_compact       the runs of every pair from its area into the flat array
 */
#include <algorithm>
#include <memory>
#include <mutex>

#include "sa_ctx.h"
#include "sa_fit_core.h"
#include "sa_traceback_core.h"

struct sa_alns {
	std::vector<sa_aln> rec;
	std::vector<uint32_t> cigar;
};

namespace {

constexpr int32_t SCORE_MIN = INT32_MIN / 2; /* reference src/bio/align.h:19 */
constexpr uint32_t TB_EQUAL = 16;            /* record bit 4: the two residue codes of the cell are equal (identities) */

/* one pair of a call, canonical orientation; the array is sorted by scratch size, largest first */
struct SaTbPair {
	int32_t lo, hi;      /* row sequence, column sequence: lo < hi                          */
	int32_t slot;        /* position in the caller's list                                   */
	int32_t flip;        /* the caller's a is hi: mirror on output                          */
	int64_t scratch_off; /* bytes into the batch's decision scratch, a multiple of 256      */
};

struct SaTbEnd {
	int32_t score, r, c, pad; /* where the walk starts: (m, n), SW: the end cell */
};

struct SaTbFillArgs {
	SaSeqStore st;
	const int32_t *sub;
	int32_t gap_pen, gap_opn, gap_ext;
	const SaTbPair *pairs; /* the batch */
	int32_t count;
	uint8_t *scratch;      /* decision scratch of the batch */
	SaTbEnd *ends;         /* [count] */
	int32_t *bnd;          /* per-wave strip boundary columns (M and X), the context's */
	int64_t bnd_stride;
};

struct SaTbWalkArgs {
	SaSeqStore st;
	const SaTbPair *pairs;
	const SaTbEnd *ends;
	int32_t count;
	const uint8_t *scratch;
	uint32_t *runs;          /* run areas of the whole call: slot t owns the words [run_off[t], run_off[t + 1]) */
	const int64_t *run_off;
	sa_aln *rec;             /* [npairs], by slot */
};

__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

/* value shifted in from lane-1 (DPP wave_shr:1, bound_ctrl off: lane 0 keeps its own and overrides it afterwards) */
__device__ __forceinline__ int32_t from_left(int32_t v)
{
	return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false);
}

template <int METHOD, bool FIT>
__global__ __launch_bounds__(256) void sa_k_trace_fill(SaTbFillArgs A)
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
		const SaTbPair P = A.pairs[q];
		const int32_t m = A.st.meta[P.lo].len, offi = A.st.meta[P.lo].off; /* rows: lo    */
		const int32_t n = A.st.meta[P.hi].len, offj = A.st.meta[P.hi].off; /* columns: hi */
		const uint8_t *ci = A.st.codes + offi;
		const uint8_t *cj = A.st.codes + offj;
		uint32_t *words = reinterpret_cast<uint32_t *>(A.scratch + P.scratch_off) + lane;
		const int32_t nstrips = (n + 63) >> 6;
		const int64_t strip_groups = sa_tb_strip_lines(m, 64) >> 2; /* 256-byte groups of a full strip */
		int32_t best = 0, best_r = 0, best_c = 0; /* SW end cell of this lane */
		if (FIT)
			best = border(n); /* FIT: the end cell of column n, row 0's to begin with (kept by the lane that owns the column) */
		int32_t h = 0;

		for (int32_t s = 0; s < nstrips; s++) {
			const int32_t c = (s << 6) + lane + 1;
			const bool colvalid = c <= n;
			const int32_t b = colvalid ? cj[c - 1] : 0;
			const int32_t width = (n - (s << 6)) < 64 ? (n - (s << 6)) : 64;
			const bool last_strip = s + 1 == nstrips;
			uint32_t *gw = words + 64 * (s * strip_groups);
			h = border(c);
			int32_t y = SCORE_MIN;
			int32_t x = SCORE_MIN;
			int32_t diag = border(c - 1);
			const int32_t steps = m + width - 1;
			uint32_t acc = 0;

			for (int32_t t = 0; t < steps; t++) {
				const int32_t r = t - lane + 1;
				int32_t lm = from_left(h);
				int32_t lx = SCORE_MIN;
				if (METHOD != SA_METHOD_NW)
					lx = from_left(x);
				if (lane == 0) {
					if (s == 0) {
						lm = FIT ? 0 : border(r); /* (FIT: the row sequence's first residues are free) */
						lx = SCORE_MIN;
					} else if (r <= m) {
						lm = bndM[r];
						if (METHOD != SA_METHOD_NW)
							lx = bndX[r];
					}
				}
				const bool valid = colvalid && r >= 1 && r <= m;
				const int32_t a = valid ? ci[r - 1] : 0;
				int32_t nm, nx = SCORE_MIN, ny = SCORE_MIN;
				uint32_t rec;
				if (METHOD == SA_METHOD_NW) {
					const int32_t match = diag + s_sub[a * SA_SUB_DIM + b];
					const int32_t del = h + g;
					const int32_t ins = lm + g;
					nm = imax(ins, imax(del, match));
					rec = sa_tb_encode_nw(nm, match, del);
				} else {
					const int32_t sd = diag + s_sub[b * SA_SUB_DIM + a];
					const int32_t xo = lm + o, yo = h + o;
					nx = imax(xo, lx + e);
					ny = imax(yo, y + e);
					nm = (METHOD == SA_METHOD_SW) ? imax(sd, 0) : sd;
					nm = imax(nx, nm);
					nm = imax(ny, nm);
					rec = sa_tb_encode_affine(METHOD == SA_METHOD_SW, nm, sd, nx, ny, xo, yo);
				}
				rec |= a == b ? TB_EQUAL : 0u;
				acc |= rec << (8 * (t & 3));
				if ((t & 3) == 3 || t + 1 == steps) { /* the wave's 256 contiguous bytes of these four steps */
					gw[64 * (t >> 2)] = acc;
					acc = 0;
				}
				diag = lm;
				if (valid) {
					h = nm;
					x = nx;
					y = ny;
					if (METHOD == SA_METHOD_SW && sa_tb_end_before(nm, r, c, best, best_r, best_c)) {
						best = nm;
						best_r = r;
						best_c = c;
					}
					if (FIT && c == n && nm > best) { /* (rows arrive in ascending order: strictly greater only) */
						best = nm;
						best_r = r;
					}
					if (lane == 63 && !last_strip) {
						bndM[r] = nm;
						if (METHOD != SA_METHOD_NW)
							bndX[r] = nx;
					}
				}
			}
			if (!last_strip)
				__threadfence_block(); /* boundary column visible to this wave's next strip */
		}

		SaTbEnd E;
		E.pad = 0;
		if (FIT) {
			E.score = __shfl(best, (n - 1) & 63, 64);
			E.r = __shfl(best_r, (n - 1) & 63, 64);
			E.c = n;
		} else if (METHOD == SA_METHOD_SW) {
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				const int32_t ov = __shfl_xor(best, d, 64), orr = __shfl_xor(best_r, d, 64), oc = __shfl_xor(best_c, d, 64);
				if (sa_tb_end_before(ov, orr, oc, best, best_r, best_c)) {
					best = ov;
					best_r = orr;
					best_c = oc;
				}
			}
			E.score = best;
			E.r = best_r;
			E.c = best_c;
		} else {
			E.score = __shfl(h, (n - 1) & 63, 64); /* M[m][n] sits in the lane owning column n */
			E.r = m;
			E.c = n;
		}
		if (lane == 0)
			A.ends[q] = E;
	}
}

constexpr int WIN_BYTES = 1024; /* 64 lanes x 16 bytes */

template <int METHOD, bool FIT>
__global__ __launch_bounds__(256) void sa_k_trace_walk(SaTbWalkArgs A)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_win[4][WIN_BYTES];
	const int lane = threadIdx.x & 63;
	uint8_t *win = s_win[threadIdx.x >> 6];
	const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);

	for (int64_t q = wave; q < A.count; q += nwaves) {
		const SaTbPair P = A.pairs[q];
		const SaTbEnd E = A.ends[q];
		const int32_t m = A.st.meta[P.lo].len;
		const bool flip = P.flip != 0;
		struct sa_tb_walk w = { E.r, E.c, SA_TB_STATE_M };
		struct sa_tb_rle rle;
		sa_tb_rle_init(&rle, A.runs + A.run_off[P.slot + 1]);
		int32_t ident = 0;
		int64_t win_lo = 0, win_hi = 0; /* the bytes [win_lo, win_hi) of the batch scratch are in LDS */

		for (;;) { /* everything here is wave-uniform */
			uint32_t rec = 0;
			if (!sa_tb_on_border(&w)) {
				const int64_t at = P.scratch_off + sa_tb_cell_offset(m, w.r, w.c);
				if (at < win_lo || at >= win_hi) {
					win_hi = (at & ~(int64_t)15) + 16;
					win_lo = win_hi - WIN_BYTES;
					const int64_t mine = win_lo + 16 * lane;
					uint4 v = make_uint4(0, 0, 0, 0);
					if (mine >= 0) /* (below the batch's first byte: never asked for) */
						v = *reinterpret_cast<const uint4 *>(A.scratch + mine);
					__builtin_amdgcn_wave_barrier();
					*reinterpret_cast<uint4 *>(win + 16 * lane) = v;
					__builtin_amdgcn_wave_barrier();
				}
				rec = win[at - win_lo];
			}
			const int op = FIT ? sa_tb_step_fit(&w, METHOD, rec) : sa_tb_step(&w, METHOD, rec);
			if (op < 0)
				break;
			if (op == SA_TB_OP_M)
				ident += (rec & TB_EQUAL) != 0;
			sa_tb_rle_push(&rle, sa_tb_mirror_op(op, flip), lane == 0);
		}
		sa_tb_rle_flush(&rle, lane == 0);
		if (lane == 0) {
			const bool empty = rle.columns == 0 && METHOD == SA_METHOD_SW;
			const int32_t lo0 = empty ? 0 : w.r, lo1 = empty ? 0 : E.r, hi0 = empty ? 0 : w.c, hi1 = empty ? 0 : E.c;
			sa_aln R;
			R.score = E.score;
			R.a_begin = flip ? hi0 : lo0;
			R.a_end = flip ? hi1 : lo1;
			R.b_begin = flip ? lo0 : hi0;
			R.b_end = flip ? lo1 : hi1;
			R.columns = rle.columns;
			R.identities = ident;
			R.cigar_len = rle.runs;
			R.cigar_off = 0; /* sa_k_trace_scan */
			A.rec[P.slot] = R;
		}
	}
}

/* cigar_off[t] = sum of cigar_len before t, in the caller's order; *total = the length of the flat array.  One workgroup:
 * the call has at most a few million pairs and the scan reads four bytes of each. */
__global__ __launch_bounds__(1024) void sa_k_trace_scan(sa_aln *rec, int64_t npairs, int64_t *total)
{
	__shared__ int64_t s_part[1024];
	__shared__ int64_t s_carry;
	const int tid = threadIdx.x;
	if (tid == 0)
		s_carry = 0;
	__syncthreads();
	for (int64_t base = 0; base < npairs; base += 1024) {
		const int64_t t = base + tid;
		const int64_t mine = t < npairs ? rec[t].cigar_len : 0;
		s_part[tid] = mine;
		__syncthreads();
		for (int d = 1; d < 1024; d <<= 1) {
			const int64_t add = tid >= d ? s_part[tid - d] : 0;
			__syncthreads();
			s_part[tid] += add;
			__syncthreads();
		}
		const int64_t carry = s_carry;
		if (t < npairs)
			rec[t].cigar_off = carry + s_part[tid] - mine;
		__syncthreads();
		if (tid == 1023)
			s_carry = carry + s_part[1023];
		__syncthreads();
	}
	if (tid == 0)
		*total = s_carry;
}

__global__ __launch_bounds__(256) void sa_k_trace_compact(const sa_aln *rec, int64_t npairs, const uint32_t *runs, const int64_t *run_off,
							   uint32_t *flat)
{
	const int lane = threadIdx.x & 63;
	const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
	for (int64_t t = wave; t < npairs; t += nwaves) {
		const int32_t len = rec[t].cigar_len;
		const uint32_t *src = runs + run_off[t + 1] - len;
		uint32_t *dst = flat + rec[t].cigar_off;
		for (int32_t k = lane; k < len; k += 64)
			dst[k] = src[k];
	}
}

std::mutex g_last_mutex;
struct Last {
	double fill = 0, walk = 0;
	int64_t cells = 0;
	int32_t batches = 0;
} g_last;

template <class T> struct DevBuf { /* released whatever way the function is left */
	T *p = nullptr;
	~DevBuf() { (void)hipFree(p); }
	bool alloc(size_t n, const char *what)
	{
		if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			sa_set_error("sa_ctx_alignments: %.2f GiB of device memory for %s cannot be allocated", (double)(n * sizeof(T)) / (double)(1 << 30), what);
			return false;
		}
		return true;
	}
};

bool check_pairs(const char *who, int32_t num, const int32_t *a, const int32_t *b, int64_t npairs)
{
	if (npairs < 0) {
		sa_set_error("%s: npairs = %lld is negative", who, (long long)npairs);
		return false;
	}
	if (npairs > 0 && (!a || !b)) {
		sa_set_error("%s: null pair list", who);
		return false;
	}
	for (int64_t t = 0; t < npairs; t++) {
		if (a[t] < 0 || a[t] >= num || b[t] < 0 || b[t] >= num) {
			sa_set_error("%s: pair %lld = (%d, %d): index out of range (%d sequences)", who, (long long)t, a[t], b[t], num);
			return false;
		}
		if (a[t] == b[t]) {
			sa_set_error("%s: pair %lld = (%d, %d): a == b, a sequence is not aligned with itself", who, (long long)t, a[t], b[t]);
			return false;
		}
	}
	return true;
}

template <int METHOD, bool FIT = false> void launch_batch(const SaTbFillArgs &f, const SaTbWalkArgs &w, int blocks, hipStream_t s, hipEvent_t mid)
{
	hipLaunchKernelGGL((sa_k_trace_fill<METHOD, FIT>), dim3(blocks), dim3(256), 0, s, f);
	(void)hipEventRecord(mid, s);
	hipLaunchKernelGGL((sa_k_trace_walk<METHOD, FIT>), dim3(blocks), dim3(256), 0, s, w);
}

/* fit: the pairs are (N + query, database sequence) of a search context whose method is NW or Gotoh, checked by the caller */
sa_alns *alignments_impl(sa_ctx *ctx, const int32_t *a, const int32_t *b, int64_t npairs, bool fit = false, const char *who = "sa_ctx_alignments")
{
	if (!ctx) {
		sa_set_error("%s: null context", who);
		return nullptr;
	}
	if (!check_pairs(who, ctx->num, a, b, npairs))
		return nullptr;
	if (npairs > INT32_MAX) {
		sa_set_error("%s: %lld pairs in one call (at most %d)", who, (long long)npairs, INT32_MAX);
		return nullptr;
	}
	auto out = std::make_unique<sa_alns>();
	out->rec.resize((size_t)npairs);
	if (npairs == 0) {
		std::lock_guard<std::mutex> g(g_last_mutex);
		g_last = Last{};
		return out.release();
	}
	SA_HIP_CHECK(hipSetDevice(ctx->device), return nullptr);

	/* the pairs in canonical orientation, largest scratch first: a batch is then homogeneous */
	std::vector<SaTbPair> pairs((size_t)npairs);
	std::vector<int64_t> bytes((size_t)npairs), run_off((size_t)npairs + 1, 0);
	int64_t cells = 0;
	for (int64_t t = 0; t < npairs; t++) {
		SaTbPair &p = pairs[(size_t)t];
		p.lo = std::min(a[t], b[t]);
		p.hi = std::max(a[t], b[t]);
		p.slot = (int32_t)t;
		p.flip = a[t] > b[t];
		p.scratch_off = 0;
		const int32_t m = ctx->meta[(size_t)p.lo].len, n = ctx->meta[(size_t)p.hi].len;
		bytes[(size_t)t] = sa_tb_pair_bytes(m, n);
		run_off[(size_t)t + 1] = run_off[(size_t)t] + m + n;
		cells += (int64_t)m * n;
	}
	std::stable_sort(pairs.begin(), pairs.end(), [&](const SaTbPair &x, const SaTbPair &y) { return bytes[(size_t)x.slot] > bytes[(size_t)y.slot]; });

	DevBuf<SaTbPair> d_pairs;
	DevBuf<SaTbEnd> d_ends;
	DevBuf<sa_aln> d_rec;
	DevBuf<int64_t> d_run_off, d_total;
	DevBuf<uint32_t> d_runs, d_flat;
	DevBuf<uint8_t> d_scratch;
	if (!d_pairs.alloc((size_t)npairs, "the pair list") || !d_ends.alloc((size_t)npairs, "the end cells") || !d_rec.alloc((size_t)npairs, "the records") ||
	    !d_run_off.alloc((size_t)npairs + 1, "the run offsets") || !d_total.alloc(1, "the run count") ||
	    !d_runs.alloc((size_t)run_off[(size_t)npairs], "the run areas"))
		return nullptr;

	/* batches: as many pairs as the cap allows, at least one */
	size_t free_b = 0, total_b = 0;
	SA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b), return nullptr);
	const int64_t largest = bytes[(size_t)pairs[0].slot];
	int64_t cap = (int64_t)(free_b - free_b / 8); /* (the flat array is at most as large as the run areas, allocated later) */
	cap -= std::min<int64_t>(cap, 4 * run_off[(size_t)npairs] + ((int64_t)64 << 20));
	if (largest > cap) {
		sa_set_error("%s: the decisions of a pair of %d x %d residues (%.2f GiB) do not fit the free device memory (%.2f GiB)", who,
			     ctx->meta[(size_t)pairs[0].lo].len, ctx->meta[(size_t)pairs[0].hi].len, (double)largest / (double)(1 << 30),
			     (double)free_b / (double)(1 << 30));
		return nullptr;
	}
	if (ctx->env.trace_batch_bytes > 0) /* (the switches as they were when the context was created) */
		cap = std::min<int64_t>(cap, ctx->env.trace_batch_bytes); /* (a pair above the cap is a batch of its own) */
	struct Batch {
		int64_t first, count, bytes;
	};
	std::vector<Batch> batches;
	for (int64_t t = 0; t < npairs; t++) {
		const int64_t need = bytes[(size_t)pairs[(size_t)t].slot];
		if (batches.empty() || batches.back().bytes + need > cap)
			batches.push_back(Batch{ t, 0, 0 });
		pairs[(size_t)t].scratch_off = batches.back().bytes;
		batches.back().count++;
		batches.back().bytes += need;
	}
	int64_t scratch_bytes = 0;
	for (const Batch &bt : batches)
		scratch_bytes = std::max(scratch_bytes, bt.bytes);
	if (!d_scratch.alloc((size_t)scratch_bytes, "the decision scratch"))
		return nullptr;

	struct Sync { /* stream and events; the stream is drained before anything above is freed (declared last) */
		hipStream_t s = nullptr;
		std::vector<hipEvent_t> ev;
		~Sync()
		{
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
			for (hipEvent_t e : ev)
				(void)hipEventDestroy(e);
		}
	} sy;
	SA_HIP_CHECK(hipStreamCreateWithFlags(&sy.s, hipStreamNonBlocking), return nullptr);
	sy.ev.resize(3 * batches.size() + 1, nullptr);
	for (hipEvent_t &e : sy.ev)
		SA_HIP_CHECK(hipEventCreate(&e), return nullptr);
	SA_HIP_CHECK(hipMemcpyAsync(d_pairs.p, pairs.data(), sizeof(SaTbPair) * (size_t)npairs, hipMemcpyHostToDevice, sy.s), return nullptr);
	SA_HIP_CHECK(hipMemcpyAsync(d_run_off.p, run_off.data(), sizeof(int64_t) * ((size_t)npairs + 1), hipMemcpyHostToDevice, sy.s), return nullptr);

	for (size_t k = 0; k < batches.size(); k++) {
		const Batch &bt = batches[k];
		SaTbFillArgs f{};
		f.st.codes = ctx->d_codes;
		f.st.meta = ctx->d_meta;
		f.st.num = ctx->num;
		f.sub = ctx->d_sub;
		f.gap_pen = ctx->sc.gap_pen;
		f.gap_opn = ctx->sc.gap_opn;
		f.gap_ext = ctx->sc.gap_ext;
		f.pairs = d_pairs.p + bt.first;
		f.count = (int32_t)bt.count;
		f.scratch = d_scratch.p;
		f.ends = d_ends.p + bt.first;
		f.bnd = ctx->d_scratch;
		f.bnd_stride = ctx->scratch_stride;
		SaTbWalkArgs w{};
		w.st = f.st;
		w.pairs = f.pairs;
		w.ends = f.ends;
		w.count = f.count;
		w.scratch = d_scratch.p;
		w.runs = d_runs.p;
		w.run_off = d_run_off.p;
		w.rec = d_rec.p;
		const int blocks = (int)std::min<int64_t>(ctx->generic_blocks, (bt.count + 3) / 4);
		SA_HIP_CHECK(hipEventRecord(sy.ev[3 * k], sy.s), return nullptr);
		switch (ctx->sc.method) {
		case SA_METHOD_NW:
			if (fit)
				launch_batch<SA_METHOD_NW, true>(f, w, blocks, sy.s, sy.ev[3 * k + 1]);
			else
				launch_batch<SA_METHOD_NW>(f, w, blocks, sy.s, sy.ev[3 * k + 1]);
			break;
		case SA_METHOD_GA:
			if (fit)
				launch_batch<SA_METHOD_GA, true>(f, w, blocks, sy.s, sy.ev[3 * k + 1]);
			else
				launch_batch<SA_METHOD_GA>(f, w, blocks, sy.s, sy.ev[3 * k + 1]);
			break;
		default:
			launch_batch<SA_METHOD_SW>(f, w, blocks, sy.s, sy.ev[3 * k + 1]);
			break;
		}
		SA_HIP_CHECK(hipGetLastError(), return nullptr);
		SA_HIP_CHECK(hipEventRecord(sy.ev[3 * k + 2], sy.s), return nullptr);
	}
	hipLaunchKernelGGL(sa_k_trace_scan, dim3(1), dim3(1024), 0, sy.s, d_rec.p, npairs, d_total.p);
	SA_HIP_CHECK(hipGetLastError(), return nullptr);
	int64_t total = 0;
	SA_HIP_CHECK(hipMemcpyAsync(&total, d_total.p, sizeof(total), hipMemcpyDeviceToHost, sy.s), return nullptr);
	SA_HIP_CHECK(hipStreamSynchronize(sy.s), return nullptr);
	if (total < 0 || total > run_off[(size_t)npairs]) {
		sa_set_error("%s: internal error: %lld runs for areas of %lld words", who, (long long)total, (long long)run_off[(size_t)npairs]);
		return nullptr;
	}
	if (!d_flat.alloc((size_t)total, "the CIGARs"))
		return nullptr;
	out->cigar.resize((size_t)total);
	const int cblocks = (int)std::min<int64_t>(256 * 8, (npairs + 3) / 4);
	hipLaunchKernelGGL(sa_k_trace_compact, dim3(cblocks), dim3(256), 0, sy.s, d_rec.p, npairs, d_runs.p, d_run_off.p, d_flat.p);
	SA_HIP_CHECK(hipGetLastError(), return nullptr);
	SA_HIP_CHECK(hipEventRecord(sy.ev.back(), sy.s), return nullptr);
	SA_HIP_CHECK(hipMemcpyAsync(out->rec.data(), d_rec.p, sizeof(sa_aln) * (size_t)npairs, hipMemcpyDeviceToHost, sy.s), return nullptr);
	if (total > 0) {
		SA_HIP_CHECK(hipMemcpyAsync(out->cigar.data(), d_flat.p, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, sy.s), return nullptr);
	}
	SA_HIP_CHECK(hipStreamSynchronize(sy.s), return nullptr);

	Last last;
	last.cells = cells;
	last.batches = (int32_t)batches.size();
	for (size_t k = 0; k < batches.size(); k++) {
		float fill_ms = 0.f, walk_ms = 0.f;
		SA_HIP_CHECK(hipEventElapsedTime(&fill_ms, sy.ev[3 * k], sy.ev[3 * k + 1]), return nullptr);
		SA_HIP_CHECK(hipEventElapsedTime(&walk_ms, sy.ev[3 * k + 1], sy.ev[3 * k + 2]), return nullptr);
		last.fill += (double)fill_ms * 1e-3;
		last.walk += (double)walk_ms * 1e-3;
	}
	float tail_ms = 0.f; /* scan + compaction (the read-back of the run count between them included) */
	SA_HIP_CHECK(hipEventElapsedTime(&tail_ms, sy.ev[3 * batches.size() - 1], sy.ev.back()), return nullptr);
	last.walk += (double)tail_ms * 1e-3;
	{
		std::lock_guard<std::mutex> g(g_last_mutex);
		g_last = last;
	}
	return out.release();
}

sa_alns *hip_alignments_impl(struct sa_input in, const struct sa_scoring *sc, const int32_t *a, const int32_t *b, int64_t npairs)
{
	if (!sc) {
		sa_set_error("sa_hip_alignments: null scoring");
		return nullptr;
	}
	if (!check_pairs("sa_hip_alignments", in.num, a, b, npairs))
		return nullptr;
	if (sa_hip_device_count() <= 0) {
		sa_set_error("No HIP devices available; libseqalign_hip has no CPU fallback");
		return nullptr;
	}
	sa_ctx *ctx = sa_ctx_create(0, in, sc);
	if (!ctx)
		return nullptr;
	sa_alns *res = alignments_impl(ctx, a, b, npairs);
	sa_ctx_destroy(ctx);
	return res;
}

/* host index arrays: query[t] in [0, the context's queries), db[t] in [0, N); the pair is (a, b) = (N + query[t], db[t]) */
sa_alns *fit_alignments_impl(sa_ctx *ctx, const int32_t *query, const int32_t *db, int64_t npairs)
{
	const char *who = "sa_ctx_fit_alignments";
	if (!sa_search_ctx_check(who, ctx))
		return nullptr;
	if (ctx->sc.method != SA_METHOD_NW && ctx->sc.method != SA_METHOD_GA) {
		sa_set_error("%s: the context's method is SW, which is local already; fit is defined for NW and Gotoh", who);
		return nullptr;
	}
	if (npairs < 0) {
		sa_set_error("%s: npairs = %lld is negative", who, (long long)npairs);
		return nullptr;
	}
	if (npairs > 0 && (!query || !db)) {
		sa_set_error("%s: null pair list", who);
		return nullptr;
	}
	std::vector<int32_t> a((size_t)npairs);
	for (int64_t t = 0; t < npairs; t++) {
		if (query[t] < 0 || query[t] >= ctx->search_queries || db[t] < 0 || db[t] >= ctx->search_db) {
			sa_set_error("%s: pair %lld = (query %d, database sequence %d): index out of range (%d queries, %d database sequences)", who, (long long)t,
				     query[t], db[t], ctx->search_queries, ctx->search_db);
			return nullptr;
		}
		a[(size_t)t] = ctx->search_db + query[t];
	}
	return alignments_impl(ctx, a.data(), db, npairs, true, who);
}

} // namespace

extern "C" sa_alns *sa_ctx_fit_alignments(sa_ctx *ctx, const int32_t *query, const int32_t *db, int64_t npairs)
{
	return sa_guard("sa_ctx_fit_alignments", (sa_alns *)nullptr, [&] { return fit_alignments_impl(ctx, query, db, npairs); });
}

extern "C" sa_alns *sa_ctx_alignments(sa_ctx *ctx, const int32_t *a, const int32_t *b, int64_t npairs)
{
	return sa_guard("sa_ctx_alignments", (sa_alns *)nullptr, [&] { return alignments_impl(ctx, a, b, npairs); });
}

extern "C" sa_alns *sa_hip_alignments(struct sa_input in, const struct sa_scoring *sc, const int32_t *a, const int32_t *b, int64_t npairs)
{
	return sa_guard("sa_hip_alignments", (sa_alns *)nullptr, [&] { return hip_alignments_impl(in, sc, a, b, npairs); });
}

extern "C" const struct sa_aln *sa_alns_records(const sa_alns *alns)
{
	return sa_guard("sa_alns_records", (const sa_aln *)nullptr, [&] { return alns ? alns->rec.data() : nullptr; });
}

extern "C" const uint32_t *sa_alns_cigar(const sa_alns *alns, int64_t *runs)
{
	return sa_guard("sa_alns_cigar", (const uint32_t *)nullptr, [&] {
		if (runs)
			*runs = alns ? (int64_t)alns->cigar.size() : 0;
		return alns ? alns->cigar.data() : nullptr;
	});
}

extern "C" int64_t sa_alns_count(const sa_alns *alns)
{
	return sa_guard("sa_alns_count", (int64_t)0, [&] { return alns ? (int64_t)alns->rec.size() : (int64_t)0; });
}

extern "C" void sa_alns_destroy(sa_alns *alns)
{
	sa_guard_void("sa_alns_destroy", [&] { delete alns; });
}

extern "C" double sa_hip_last_alignments_seconds(void)
{
	return sa_guard("sa_hip_last_alignments_seconds", 0.0, [&] {
		std::lock_guard<std::mutex> g(g_last_mutex);
		return g_last.fill + g_last.walk;
	});
}

extern "C" void sa_hip_last_alignments_breakdown(double *fill_seconds, double *walk_seconds, int64_t *cells, int32_t *batches)
{
	sa_guard_void("sa_hip_last_alignments_breakdown", [&] {
		std::lock_guard<std::mutex> g(g_last_mutex);
		if (fill_seconds)
			*fill_seconds = g_last.fill;
		if (walk_seconds)
			*walk_seconds = g_last.walk;
		if (cells)
			*cells = g_last.cells;
		if (batches)
			*batches = g_last.batches;
	});
}
