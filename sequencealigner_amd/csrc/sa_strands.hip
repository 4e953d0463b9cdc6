/*
 * sa_strands.hip -- both strands of DNA queries: the fold of the forward and the reverse-complement rows of a strands context
 * and the strand of every hit (sa_ctx_strand_fold, sa_ctx_hits_strand, sa_ctx_hits_above_strand, sa_hip_search_strands).  No
 * reference counterpart.  The contract is in include/seqalign_hip.h; the complement table, the bitmap geometry, the fold rule,
 * the segment rule and the serial restatement are in sa_strands_core.h, which the host compiles as well.
 *
 * A strands context (sa_context.hip: sa_ctx_create_search_strands) is an ordinary search context whose query rows are the M
 * queries followed by their M reverse complements: every existing search call serves both halves, and no alignment kernel
 * knows of strands.  What is new runs where the two rectangles already are:
 *   sa_k_strand_fold<SCORES>  streaming: wave w of the grid folds segment w % S of row w / S, 64 consecutive d per step, ST_DEPTH
 *                             steps per group with every load of the group issued before the first use.  A lane reads its
 *                             cell of both value rectangles (and of both raw-score rectangles), keeps the larger value -- the
 *                             forward one on a tie -- and writes it; the ballot of "reverse" over the wave is one word of the
 *                             bitmap, which lane 0 writes.  Segment bounds are multiples of 64: no word has two writers.  Every
 *                             cell is read and written by the same lane, once: in place is as good as disjoint.  Loads are one
 *                             dword per lane, 256 contiguous bytes per wave instruction: a row begins at byte 4 r N, any dword
 *                             alignment, and a ballot word wants one d per lane, so nothing wider fits the layout.
 *   sa_k_hits_strand          one thread per hit of an M x k list: the bit of (row, index), 255 outside [0, N).
 *   sa_k_hits_above_strand    the same over a CSR: wave w takes part w % S of the entries of row w / S, whose bounds it reads from
 *                             the 64-bit offsets on the device -- E is never known to the host here.
 * No kernel shares state between waves, none uses atomics: the same input gives the same bytes.
 */
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

#include "sa_ctx.h"
#include "sa_strands_core.h"

namespace {

constexpr int ST_THREADS = 256; /* four waves */
constexpr int ST_DEPTH = 4;     /* steps of 64 cells whose loads are in flight together (sa_search_above.hip: AB_DEPTH) */

/* (no __restrict__ on the rectangles: vbest may be vfwd, sbest may be sfwd) */
template <bool SCORES>
__global__ __launch_bounds__(ST_THREADS) void sa_k_strand_fold(const int32_t *vfwd, const int32_t *vrev, const int32_t *sfwd, const int32_t *srev,
								int32_t n_db, int32_t nq, int32_t S, int32_t *vbest, int32_t *sbest,
								uint64_t *__restrict__ bits)
{
	const int lane = threadIdx.x & 63;
	const int64_t w = (int64_t)blockIdx.x * (ST_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (w >= (int64_t)nq * S) /* (wave-uniform) */
		return;
	const int64_t r = w / S;
	const int32_t seg = (int32_t)(w - r * S);
	const int64_t c0 = sa_strand_seg_begin(n_db, S, seg), c1 = sa_strand_seg_begin(n_db, S, seg + 1); /* c0: a multiple of 64 */
	const int64_t row_at = r * (int64_t)n_db;
	uint64_t *const brow = bits ? bits + r * sa_strand_words(n_db) : nullptr;
	for (int64_t b = c0; b < c1; b += ST_DEPTH * 64) { /* (64-bit: b + a group may pass INT32_MAX) */
		int32_t vf[ST_DEPTH], vr[ST_DEPTH], sf[ST_DEPTH], sr[ST_DEPTH];
#pragma unroll
		for (int u = 0; u < ST_DEPTH; u++) {
			const int64_t c = b + u * 64 + lane;
			const bool in = c < c1;
			vf[u] = in ? vfwd[row_at + c] : 0;
			vr[u] = in ? vrev[row_at + c] : 0;
			if (SCORES) {
				sf[u] = in ? sfwd[row_at + c] : 0;
				sr[u] = in ? srev[row_at + c] : 0;
			}
		}
#pragma unroll
		for (int u = 0; u < ST_DEPTH; u++) {
			const int64_t c = b + u * 64 + lane;
			const bool in = c < c1;
			const bool rev = in && sa_strand_pick(vf[u], vr[u]) == SA_STRAND_REVERSE;
			const uint64_t word = __ballot(rev); /* lanes beyond the row's end: 0 */
			if (in) {
				vbest[row_at + c] = rev ? vr[u] : vf[u];
				if (SCORES)
					sbest[row_at + c] = rev ? sr[u] : sf[u];
			}
			if (brow && lane == 0 && b + u * 64 < c1)
				brow[(b + u * 64) >> 6] = word;
		}
	}
}

__global__ __launch_bounds__(256) void sa_k_hits_strand(const uint64_t *__restrict__ bits, int32_t n_db, int32_t nq, int32_t k,
							 const int32_t *__restrict__ index, uint8_t *__restrict__ strand)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t < (int64_t)nq * k)
		strand[t] = sa_strand_bit(bits + t / k * sa_strand_words(n_db), n_db, index[t]);
}

/* wave w: part w % S of the entries [offsets[r], offsets[r + 1]) of row r = w / S, the entries dealt evenly */
__global__ __launch_bounds__(ST_THREADS) void sa_k_hits_above_strand(const uint64_t *__restrict__ bits, int32_t n_db, int32_t nq, int32_t S,
								      const int64_t *__restrict__ offsets, const int32_t *__restrict__ index,
								      uint8_t *__restrict__ strand)
{
	const int lane = threadIdx.x & 63;
	const int64_t w = (int64_t)blockIdx.x * (ST_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (w >= (int64_t)nq * S) /* (wave-uniform) */
		return;
	const int64_t r = w / S, part = w - r * S;
	const int64_t begin = offsets[r], count = offsets[r + 1] - begin;
	if (count <= 0)
		return;
	/* (count <= N < 2^31 for offsets that sa_ctx_hits_above_offsets made, S <= 8192: the products fit 64 bits with room to spare;
	 * offsets of any other origin are the caller's) */
	const int64_t e0 = begin + count * part / S, e1 = begin + count * (part + 1) / S;
	const uint64_t *brow = bits + r * sa_strand_words(n_db);
	for (int64_t e = e0 + lane; e < e1; e += 64)
		strand[e] = sa_strand_bit(brow, n_db, index[e]);
}

std::atomic<double> g_last_strands_seconds{ 0.0 };

int fold_launch(const int32_t *vf, const int32_t *vr, const int32_t *sf, const int32_t *sr, int32_t n_db, int32_t nq, int32_t *vbest, int32_t *sbest,
		uint64_t *bits, hipStream_t s)
{
	const int32_t S = sa_strand_segments(n_db, nq);
	constexpr int WPB = ST_THREADS / 64;
	const int64_t waves = (int64_t)nq * S;
	const dim3 grid((unsigned)((waves + WPB - 1) / WPB));
	if (sf)
		hipLaunchKernelGGL(sa_k_strand_fold<true>, grid, dim3(ST_THREADS), 0, s, vf, vr, sf, sr, n_db, nq, S, vbest, sbest, bits);
	else
		hipLaunchKernelGGL(sa_k_strand_fold<false>, grid, dim3(ST_THREADS), 0, s, vf, vr, sf, sr, n_db, nq, S, vbest, sbest, bits);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

int hits_strand_launch(const uint64_t *bits, int32_t n_db, int32_t nq, int32_t k, const int32_t *index, uint8_t *strand, hipStream_t s)
{
	const int64_t hits = (int64_t)nq * k;
	hipLaunchKernelGGL(sa_k_hits_strand, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, s, bits, n_db, nq, k, index, strand);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

int above_strand_launch(const uint64_t *bits, int32_t n_db, int32_t nq, const int64_t *offsets, const int32_t *index, uint8_t *strand, hipStream_t s)
{
	const int32_t S = sa_strand_segments(n_db, nq);
	constexpr int WPB = ST_THREADS / 64;
	const int64_t waves = (int64_t)nq * S;
	hipLaunchKernelGGL(sa_k_hits_above_strand, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(ST_THREADS), 0, s, bits, n_db, nq, S, offsets, index,
			   strand);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

/* what the three device-resident calls refuse alike; M = the queries of the strands context */
bool strands_check(const char *who, const sa_ctx *ctx, int32_t nq, const void *d_bits)
{
	if (!sa_search_ctx_check(who, ctx))
		return false;
	if (ctx->search_strands != 2) {
		sa_set_error("%s: not a strands context (sa_ctx_create_search_strands)", who);
		return false;
	}
	const int32_t m = ctx->search_queries / 2;
	if (nq < 1 || nq > m) {
		sa_set_error("%s: %d rows, the context has %d queries on two strands: nq must be in [1, %d]", who, nq, m, m);
		return false;
	}
	if (reinterpret_cast<uintptr_t>(d_bits) % alignof(uint64_t)) {
		sa_set_error("%s: d_bits not 8-byte aligned", who);
		return false;
	}
	return true;
}

struct DevBuf {
	void *p = nullptr;
	~DevBuf() { (void)hipFree(p); }
	bool alloc(const char *who, size_t bytes, const char *what)
	{
		if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			sa_set_error("%s: %s (%.2f GiB) does not fit the device's memory", who, what, (double)bytes / (double)(1 << 30));
			return false;
		}
		return true;
	}
};

struct Want {
	int32_t *index, *value, *score;
	uint8_t *strand;
	int32_t *rect, *vrect;
	uint8_t *srect;
};

/* what a strands context would refuse, said before a device is looked for */
bool inputs_check(const char *who, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp)
{
	if ((int64_t)db.num + 2 * (int64_t)queries.num > INT32_MAX) {
		sa_set_error("%s: %lld sequences exceed 32-bit sequence indices", who, (long long)db.num + 2 * (long long)queries.num);
		return false;
	}
	int64_t bytes = 0;
	for (int32_t k = 0; k < db.num; k++)
		bytes += (int64_t)std::max<int32_t>(db.meta[k].len, 0) + 1;
	for (int32_t k = 0; k < queries.num; k++) {
		const sa_meta m = queries.meta[k];
		if (m.len < 1 || m.off < 0) {
			sa_set_error("Query sequence #%d has invalid offset/length (%d/%d)", k + 1, m.off, m.len);
			return false;
		}
		bytes += 2 * ((int64_t)m.len + 1);
	}
	if (bytes > INT32_MAX) {
		sa_set_error("%s: the concatenated sequence store exceeds 2 GiB", who);
		return false;
	}
	return sa_strands_rc_checked(who, queries, comp, sc);
}

/* norm != NULL: normalised scores; pid_denom != NULL: percent identity; neither: raw scores */
bool strands_impl(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp_in, int32_t k, const Want &w,
		  const struct sa_norm *norm, const int32_t *pid_denom)
{
	const char *who = "sa_hip_search_strands";
	if (!sc) {
		sa_set_error("%s: null argument", who);
		return false;
	}
	if (norm && pid_denom) {
		sa_set_error("%s: norm and pid_denom exclude each other", who);
		return false;
	}
	const bool want_hits = w.index || w.value || w.score || w.strand;
	if (want_hits && !w.index) {
		sa_set_error("%s: value, score and strand belong to the hits of index, which is null", who);
		return false;
	}
	if (!want_hits && !w.rect && !w.vrect && !w.srect) {
		sa_set_error("%s: nothing asked for (index, rect, vrect and srect are all null)", who);
		return false;
	}
	if (db.num < 1 || queries.num < 1) {
		sa_set_error("%s: empty store (%d database sequences, %d queries; min: 1 each)", who, db.num, queries.num);
		return false;
	}
	if (!db.seqs || !db.meta || !queries.seqs || !queries.meta) {
		sa_set_error("%s: null sequence store", who);
		return false;
	}
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	if (norm && !sa_norm_check(who, norm))
		return false;
	if (pid_denom && !sa_identity_denom_check(who, *pid_denom))
		return false;
	uint8_t dna[SA_LUT_SIZE];
	sa_strands_complement_table(dna);
	const uint8_t *comp = comp_in ? comp_in : dna;
	if (!inputs_check(who, db, queries, sc, comp))
		return false;
	if (sa_hip_device_count() <= 0) {
		sa_set_error("No HIP devices available; libseqalign_hip has no CPU fallback");
		return false;
	}
	struct Ctx {
		sa_ctx *c = nullptr;
		~Ctx() { sa_ctx_destroy(c); }
	} cx;
	cx.c = sa_ctx_create_search_strands(0, db, queries, sc, comp);
	if (!cx.c)
		return false;
	sa_ctx *ctx = cx.c;
	const int64_t n = db.num, m = queries.num, words = sa_strand_words(n);
	const bool quantity = norm || pid_denom, aligned = !pid_denom;
	/* Batch: as sa_hip_search_norm / _pid size it, with both strands counted.  Per query: the range row (the longest, N + 2 M - 1
	 * elements; the two halves of a batch use the one buffer in turn; none under percent identity), a forward and a reverse row of
	 * each rectangle, a row of the bitmap, and with hits index, value, score, one partial list and the strands. */
	if (pid_denom && !sa_identity_payload_scratch(ctx))
		return false;
	size_t free_b = 0, total_b = 0;
	SA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b), return false);
	const int64_t per_query = (aligned ? 4 * (n + 2 * m) : 0) + (quantity ? 16 : 8) * n + 8 * words + (want_hits ? 21 * (int64_t)k : 0);
	int64_t budget = (int64_t)(free_b - free_b / 4);
	if (ctx->env.search_batch_bytes > 0)
		budget = std::min<int64_t>(budget, ctx->env.search_batch_bytes);
	const int32_t nqb = (int32_t)std::max<int64_t>(1, std::min<int64_t>(m, budget / per_query));
	size_t range_bytes = 0, part_bytes = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = (int32_t)std::min<int64_t>(nqb, m - q0);
		if (aligned) /* (the reverse half begins M queries later: its range is the longer one) */
			range_bytes = std::max(range_bytes, sa_search_scratch_bytes(ctx, (int32_t)(m + q0), nq));
		if (want_hits)
			part_bytes = std::max(part_bytes, sa_hits_scratch_bytes((int32_t)n, nq, k));
	}
	const size_t rect_bytes = sizeof(int32_t) * (size_t)nqb * (size_t)n, cap = want_hits ? (size_t)nqb * (size_t)k : 0;
	DevBuf d_range, d_den, d_rf, d_rr, d_vf, d_vr, d_bits, d_hits, d_strand, d_part;
	if ((aligned && !d_range.alloc(who, range_bytes, "the packed range of a query batch")) ||
	    (norm && !d_den.alloc(who, sizeof(int32_t) * (size_t)(n + 2 * m), "the denominators")) ||
	    !d_rf.alloc(who, rect_bytes, "the forward rectangle of a query batch") || !d_rr.alloc(who, rect_bytes, "the reverse rectangle of a query batch") ||
	    (quantity && (!d_vf.alloc(who, rect_bytes, "the forward value rectangle of a query batch") ||
			  !d_vr.alloc(who, rect_bytes, "the reverse value rectangle of a query batch"))) ||
	    !d_bits.alloc(who, sizeof(uint64_t) * (size_t)nqb * (size_t)words, "the strand bitmap of a query batch") ||
	    (want_hits && (!d_hits.alloc(who, 3 * sizeof(int32_t) * cap, "the hits of a query batch") || !d_strand.alloc(who, cap, "the strands of the hits") ||
			   !d_part.alloc(who, part_bytes, "the partial hit lists"))))
		return false;
	struct Sync { /* the stream is drained before the buffers above are freed (declared after them) */
		hipStream_t s = nullptr;
		/* start, forward range aligned, its rows moved, reverse range aligned, its rows moved, values done, folded, hits taken, strands taken */
		hipEvent_t ev[9] = {};
		~Sync()
		{
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
			for (hipEvent_t e : ev)
				if (e)
					(void)hipEventDestroy(e);
		}
	} sy;
	SA_HIP_CHECK(hipStreamCreateWithFlags(&sy.s, hipStreamNonBlocking), return false);
	for (hipEvent_t &e : sy.ev)
		SA_HIP_CHECK(hipEventCreate(&e), return false);
	std::vector<int32_t> h_den(norm && norm->denominators ? (size_t)(n + 2 * m) : 0);
	std::vector<uint64_t> h_bits(w.srect ? (size_t)nqb * (size_t)words : 0);
	double t_align = 0.0, t_gather = 0.0, t_quantity = 0.0, t_hits = 0.0, t_strands = 0.0;
	int32_t batches = 0;
	for (int64_t q0 = 0; q0 < m; q0 += nqb) {
		const int32_t nq = (int32_t)std::min<int64_t>(nqb, m - q0);
		const size_t hits = want_hits ? (size_t)nq * (size_t)k : 0, elems = (size_t)nq * (size_t)n;
		int32_t *const rf = static_cast<int32_t *>(d_rf.p), *const rr = static_cast<int32_t *>(d_rr.p);
		int32_t *const vf = quantity ? static_cast<int32_t *>(d_vf.p) : rf, *const vr = quantity ? static_cast<int32_t *>(d_vr.p) : rr;
		uint64_t *const db_bits = static_cast<uint64_t *>(d_bits.p);
		int32_t *const di = static_cast<int32_t *>(d_hits.p), *const dval = di ? di + cap : nullptr, *const dsc = di ? di + 2 * cap : nullptr;
		uint8_t *const dst = static_cast<uint8_t *>(d_strand.p);
		const int32_t *const den = static_cast<const int32_t *>(d_den.p);
		SA_HIP_CHECK(hipEventRecord(sy.ev[0], sy.s), return false);
		if (aligned) {
			if (sa_search_range_launch(ctx, (int32_t)q0, nq, rf, d_range.p, sy.s, sy.ev[1]) != 0)
				return false;
			SA_HIP_CHECK(hipEventRecord(sy.ev[2], sy.s), return false);
			if (sa_search_range_launch(ctx, (int32_t)(m + q0), nq, rr, d_range.p, sy.s, sy.ev[3]) != 0)
				return false;
			SA_HIP_CHECK(hipEventRecord(sy.ev[4], sy.s), return false);
			if (norm) {
				if (q0 == 0) { /* once per call */
					SA_HIP_CHECK(sa_denominators_launch(ctx, norm->source, static_cast<int32_t *>(d_den.p), sy.s), return false);
				}
				if (sa_normalize_rect_launch(rf, (int32_t)n, (int32_t)q0, nq, den, norm->rule, vf, sy.s) != 0 ||
				    sa_normalize_rect_launch(rr, (int32_t)n, (int32_t)(m + q0), nq, den, norm->rule, vr, sy.s) != 0)
					return false;
			}
		} else {
			const struct sa_identity_out fwd = { rf, nullptr, nullptr, vf, *pid_denom }, rev = { rr, nullptr, nullptr, vr, *pid_denom };
			for (int t = 1; t <= 4; t++)
				SA_HIP_CHECK(hipEventRecord(sy.ev[t], sy.s), return false);
			if (!sa_identity_rect(who, ctx, (int32_t)q0, nq, &fwd, sy.s) || !sa_identity_rect(who, ctx, (int32_t)(m + q0), nq, &rev, sy.s))
				return false;
		}
		SA_HIP_CHECK(hipEventRecord(sy.ev[5], sy.s), return false);
		/* in place: the folded values replace the forward values, the folded raw scores the forward raw scores */
		if (fold_launch(vf, vr, quantity ? rf : nullptr, quantity ? rr : nullptr, (int32_t)n, nq, vf, quantity ? rf : nullptr, db_bits, sy.s) != 0)
			return false;
		SA_HIP_CHECK(hipEventRecord(sy.ev[6], sy.s), return false);
		if (want_hits && (sa_hits_launch(vf, (int32_t)n, nq, k, di, dval, d_part.p, sy.s) != 0 ||
				  (quantity && sa_hits_take_launch(rf, (int32_t)n, nq, k, di, dsc, sy.s) != 0)))
			return false;
		SA_HIP_CHECK(hipEventRecord(sy.ev[7], sy.s), return false);
		if (want_hits && w.strand && hits_strand_launch(db_bits, (int32_t)n, nq, k, di, dst, sy.s) != 0)
			return false;
		SA_HIP_CHECK(hipEventRecord(sy.ev[8], sy.s), return false);
		if (want_hits) {
			SA_HIP_CHECK(hipMemcpyAsync(w.index + q0 * k, di, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, sy.s), return false);
			if (w.value) {
				SA_HIP_CHECK(hipMemcpyAsync(w.value + q0 * k, dval, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, sy.s), return false);
			}
			if (w.score) { /* (raw scores: the value is the score) */
				SA_HIP_CHECK(hipMemcpyAsync(w.score + q0 * k, quantity ? dsc : dval, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, sy.s),
					     return false);
			}
			if (w.strand) {
				SA_HIP_CHECK(hipMemcpyAsync(w.strand + q0 * k, dst, hits, hipMemcpyDeviceToHost, sy.s), return false);
			}
		}
		if (w.rect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.rect + q0 * n, rf, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return false);
		}
		if (w.vrect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.vrect + q0 * n, vf, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, sy.s), return false);
		}
		if (w.srect) {
			SA_HIP_CHECK(hipMemcpyAsync(h_bits.data(), db_bits, sizeof(uint64_t) * (size_t)nq * (size_t)words, hipMemcpyDeviceToHost, sy.s),
				     return false);
		}
		if (q0 == 0 && !h_den.empty()) {
			SA_HIP_CHECK(hipMemcpyAsync(h_den.data(), d_den.p, sizeof(int32_t) * h_den.size(), hipMemcpyDeviceToHost, sy.s), return false);
		}
		SA_HIP_CHECK(hipStreamSynchronize(sy.s), return false); /* (the next batch reuses the buffers) */
		if (w.srect) /* the bitmap crossed the bus, one byte per cell is what the caller reads */
			for (int64_t r = 0; r < nq; r++)
				for (int64_t d = 0; d < n; d++)
					w.srect[(q0 + r) * n + d] = sa_strand_bit(h_bits.data() + r * words, (int32_t)n, (int32_t)d);
		float ms[8] = {};
		for (int t = 0; t < 8; t++)
			SA_HIP_CHECK(hipEventElapsedTime(&ms[t], sy.ev[t], sy.ev[t + 1]), return false);
		t_align += ((double)ms[0] + (double)ms[2]) * 1e-3;
		t_gather += ((double)ms[1] + (double)ms[3]) * 1e-3;
		t_quantity += (double)ms[4] * 1e-3;
		t_strands += ((double)ms[5] + (double)ms[7]) * 1e-3;
		t_hits += (double)ms[6] * 1e-3;
		batches++;
	}
	if (!h_den.empty())
		std::copy(h_den.begin(), h_den.end(), norm->denominators);
	g_last_strands_seconds.store(t_strands);
	sa_search_quantity_last_set(quantity ? t_quantity : 0.0);
	/* (under percent identity the sweeps are the alignment as well: they are what delivers the scores) */
	sa_search_last_set(aligned ? t_align : t_quantity, t_gather, t_hits, batches);
	return true;
}

} // namespace

/* for sa_search_above.hip (sa_ctx.h) */
bool sa_strands_inputs_check(const char *who, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp)
{
	return inputs_check(who, db, queries, sc, comp);
}
int sa_strand_fold_launch(const int32_t *vf, const int32_t *vr, const int32_t *sf, const int32_t *sr, int32_t n_db, int32_t nq, int32_t *vbest,
			  int32_t *sbest, uint64_t *bits, hipStream_t s)
{
	return fold_launch(vf, vr, sf, sr, n_db, nq, vbest, sbest, bits, s);
}
int sa_hits_above_strand_launch(const uint64_t *bits, int32_t n_db, int32_t nq, const int64_t *offsets, const int32_t *index, uint8_t *strand,
				hipStream_t s)
{
	return above_strand_launch(bits, n_db, nq, offsets, index, strand, s);
}
void sa_strands_last_set(double seconds) { g_last_strands_seconds.store(seconds); }

/* for sa_context.hip and the one-call forms (sa_ctx.h) */
bool sa_strands_rc_checked(const char *who, struct sa_input in, const uint8_t *comp, const struct sa_scoring *sc)
{
	int32_t seq = 0, pos = 0;
	uint8_t byte = 0;
	const int why = sa_strands_rc_check(in, comp, sc ? sc->lut : nullptr, &seq, &pos, &byte);
	if (why == SA_RC_OK)
		return true;
	const bool print = byte >= 0x21 && byte < 0x7f;
	if (why == SA_RC_NO_COMPLEMENT)
		sa_set_error("%s: sequence #%d has no reverse complement: residue %d is byte 0x%02x%s%c%s, which has no complement", who, seq + 1, pos + 1,
			     byte, print ? " ('" : "", print ? byte : ' ', print ? "')" : "");
	else
		sa_set_error("%s: sequence #%d has no reverse complement: residue %d is byte 0x%02x%s%c%s, whose complement '%c' the scoring's "
			     "alphabet does not hold",
			     who, seq + 1, pos + 1, byte, print ? " ('" : "", print ? byte : ' ', print ? "')" : "", comp[byte]);
	return false;
}

extern "C" void sa_dna_complement(uint8_t comp[SA_LUT_SIZE])
{
	sa_guard_void("sa_dna_complement", [&] {
		if (comp)
			sa_strands_complement_table(comp);
	});
}

extern "C" bool sa_reverse_complement(struct sa_input in, const uint8_t *comp, const struct sa_scoring *sc, uint8_t *blob_out)
{
	return sa_guard("sa_reverse_complement", false, [&] {
		const char *who = "sa_reverse_complement";
		if (in.num < 0 || (in.num > 0 && (!in.seqs || !in.meta)) || !blob_out) {
			sa_set_error("%s: null argument", who);
			return false;
		}
		if (blob_out == in.seqs) {
			sa_set_error("%s: blob_out is the input blob: the reverse complement is not made in place", who);
			return false;
		}
		for (int32_t k = 0; k < in.num; k++)
			if (in.meta[k].len < 0 || in.meta[k].off < 0) {
				sa_set_error("Sequence #%d has invalid offset/length (%d/%d)", k + 1, in.meta[k].off, in.meta[k].len);
				return false;
			}
		uint8_t dna[SA_LUT_SIZE];
		sa_strands_complement_table(dna);
		if (!comp)
			comp = dna;
		if (!sa_strands_rc_checked(who, in, comp, sc))
			return false;
		sa_strands_rc_write(in, comp, blob_out);
		return true;
	});
}

extern "C" int sa_ctx_strand_fold(sa_ctx *ctx, const int32_t *d_vfwd, const int32_t *d_vrev, const int32_t *d_sfwd, const int32_t *d_srev, int32_t nq,
				  int32_t *d_vbest, int32_t *d_sbest, uint64_t *d_bits, void *stream)
{
	return sa_guard("sa_ctx_strand_fold", 1, [&] {
		const char *who = "sa_ctx_strand_fold";
		if (!strands_check(who, ctx, nq, d_bits))
			return 1;
		if (!d_vfwd || !d_vrev || !d_vbest) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if ((d_sfwd || d_srev || d_sbest) && (!d_sfwd || !d_srev || !d_sbest)) {
			sa_set_error("%s: d_sfwd, d_srev and d_sbest go together: all three or none", who);
			return 1;
		}
		if ((uintptr_t)d_vfwd % 4 || (uintptr_t)d_vrev % 4 || (uintptr_t)d_vbest % 4 || (uintptr_t)d_sfwd % 4 || (uintptr_t)d_srev % 4 ||
		    (uintptr_t)d_sbest % 4) {
			sa_set_error("%s: the rectangles want 4-byte alignment", who);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return fold_launch(d_vfwd, d_vrev, d_sfwd, d_srev, ctx->search_db, nq, d_vbest, d_sbest, d_bits, (hipStream_t)stream);
	});
}

extern "C" int sa_ctx_hits_strand(sa_ctx *ctx, const uint64_t *d_bits, int32_t nq, int32_t k, const int32_t *d_index, uint8_t *d_strand, void *stream)
{
	return sa_guard("sa_ctx_hits_strand", 1, [&] {
		const char *who = "sa_ctx_hits_strand";
		if (!strands_check(who, ctx, nq, d_bits))
			return 1;
		if (!d_bits || !d_index || !d_strand) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if (!sa_hits_check(who, ctx->search_db, nq, k))
			return 1;
		if ((uintptr_t)d_index % 4) {
			sa_set_error("%s: d_index wants 4-byte alignment", who);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return hits_strand_launch(d_bits, ctx->search_db, nq, k, d_index, d_strand, (hipStream_t)stream);
	});
}

extern "C" int sa_ctx_hits_above_strand(sa_ctx *ctx, const uint64_t *d_bits, int32_t nq, const int64_t *d_offsets, const int32_t *d_index,
					uint8_t *d_strand, void *stream)
{
	return sa_guard("sa_ctx_hits_above_strand", 1, [&] {
		const char *who = "sa_ctx_hits_above_strand";
		if (!strands_check(who, ctx, nq, d_bits))
			return 1;
		if (!d_bits || !d_offsets || !d_index || !d_strand) {
			sa_set_error("%s: null argument", who);
			return 1;
		}
		if ((uintptr_t)d_offsets % 8 || (uintptr_t)d_index % 4) {
			sa_set_error("%s: d_offsets wants 8-byte and d_index 4-byte alignment", who);
			return 1;
		}
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		return above_strand_launch(d_bits, ctx->search_db, nq, d_offsets, d_index, d_strand, (hipStream_t)stream);
	});
}

extern "C" bool sa_hip_search_strands(struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp, int32_t k,
				      int32_t *index, int32_t *value, int32_t *score, uint8_t *strand, int32_t *rect, int32_t *vrect, uint8_t *srect,
				      const struct sa_norm *norm, const int32_t *pid_denom)
{
	return sa_guard("sa_hip_search_strands", false, [&] {
		const Want w = { index, value, score, strand, rect, vrect, srect };
		return strands_impl(db, queries, sc, comp, k, w, norm, pid_denom);
	});
}

extern "C" double sa_hip_last_search_strands_seconds(void)
{
	return sa_guard("sa_hip_last_search_strands_seconds", 0.0, [&] { return g_last_strands_seconds.load(); });
}
