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

#include "sa_search_run.h"
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

} // namespace

/* the launches of sa_ctx_strand_fold and sa_ctx_hits_above_strand, their arguments checked by the caller */
int sa_strand_fold_launch(const int32_t *vf, const int32_t *vr, const int32_t *sf, const int32_t *sr, int32_t n_db, int32_t nq, int32_t *vbest,
			  int32_t *sbest, uint64_t *bits, hipStream_t s)
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

int sa_hits_above_strand_launch(const uint64_t *bits, int32_t n_db, int32_t nq, const int64_t *offsets, const int32_t *index, uint8_t *strand,
				hipStream_t s)
{
	const int32_t S = sa_strand_segments(n_db, nq);
	constexpr int WPB = ST_THREADS / 64;
	const int64_t waves = (int64_t)nq * S;
	hipLaunchKernelGGL(sa_k_hits_above_strand, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(ST_THREADS), 0, s, bits, n_db, nq, S, offsets, index,
			   strand);
	SA_HIP_CHECK(hipGetLastError(), return 1);
	return 0;
}

void sa_strands_last_set(double seconds) { g_last_strands_seconds.store(seconds); }

/* what a strands context would refuse, said before a device is looked for */
bool sa_strands_inputs_check(const char *who, struct sa_input db, struct sa_input queries, const struct sa_scoring *sc, const uint8_t *comp)
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

namespace {

int hits_strand_launch(const uint64_t *bits, int32_t n_db, int32_t nq, int32_t k, const int32_t *index, uint8_t *strand, hipStream_t s)
{
	const int64_t hits = (int64_t)nq * k;
	hipLaunchKernelGGL(sa_k_hits_strand, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, s, bits, n_db, nq, k, index, strand);
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

struct Want {
	int32_t *index, *value, *score;
	uint8_t *strand;
	int32_t *rect, *vrect;
	uint8_t *srect;
};

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
	if (!sa_run_stores_not_empty(who, db, queries) || !sa_run_stores_not_null(who, db, queries))
		return false;
	if (want_hits && !sa_hits_check(who, db.num, queries.num, k))
		return false;
	if (norm && !sa_norm_check(who, norm))
		return false;
	if (pid_denom && !sa_identity_denom_check(who, *pid_denom))
		return false;
	uint8_t dna[SA_LUT_SIZE];
	sa_strands_complement_table(dna);
	const uint8_t *comp = comp_in ? comp_in : dna;
	if (!sa_strands_inputs_check(who, db, queries, sc, comp) || !sa_run_device_check())
		return false;
	SearchRun run(who);
	if (!run.adopt(sa_ctx_create_search_strands(0, db, queries, sc, comp), db, queries))
		return false;
	RectStage stage(run, norm, pid_denom, true);
	if (!stage.begin(sa_batch_tail_topk(want_hits, stage.quantity, true, k), true))
		return false;
	const int32_t n = (int32_t)run.n;
	const int64_t words = sa_strand_words(n);
	const bool quantity = stage.quantity;
	const size_t cap = want_hits ? (size_t)run.nqb * (size_t)k : 0;
	int32_t *di = nullptr;
	uint8_t *dst = nullptr;
	void *d_part = nullptr;
	if (want_hits && (!run.alloc(di, 3 * sizeof(int32_t) * cap, "the hits of a query batch") || !run.alloc(dst, cap, "the strands of the hits") ||
			  !run.alloc(d_part, run.largest([&](int32_t, int32_t nq) { return sa_hits_scratch_bytes(n, nq, k); }), "the partial hit lists")))
		return false;
	int32_t *const dval = di ? di + cap : nullptr, *const dsc = di ? di + 2 * cap : nullptr;
	int32_t *const rf = stage.raw(), *const vf = stage.value();
	if (!run.start())
		return false;
	std::vector<uint64_t> h_bits(w.srect ? (size_t)run.nqb * (size_t)words : 0);
	const bool ok = run.each_batch([&](int64_t q0, int32_t nq) {
		hipStream_t s = run.sy.s;
		const size_t hits = want_hits ? (size_t)nq * (size_t)k : 0, elems = (size_t)nq * (size_t)n;
		if (!stage.launch(q0, nq))
			return false;
		if (want_hits && (!run.stamp(SA_PH_SELECT) || sa_hits_launch(vf, n, nq, k, di, dval, d_part, s) != 0 ||
				  (quantity && sa_hits_take_launch(rf, n, nq, k, di, dsc, s) != 0)))
			return false;
		if (want_hits && w.strand && (!run.stamp(SA_PH_STRAND_TAKE) || hits_strand_launch(stage.bits(), n, nq, k, di, dst, s) != 0))
			return false;
		if (!run.stamp(SA_PH_END))
			return false;
		if (want_hits) {
			SA_HIP_CHECK(hipMemcpyAsync(w.index + q0 * k, di, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, s), return false);
			if (w.value) {
				SA_HIP_CHECK(hipMemcpyAsync(w.value + q0 * k, dval, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, s), return false);
			}
			if (w.score) { /* (raw scores: the value is the score) */
				SA_HIP_CHECK(hipMemcpyAsync(w.score + q0 * k, quantity ? dsc : dval, sizeof(int32_t) * hits, hipMemcpyDeviceToHost, s), return false);
			}
			if (w.strand) {
				SA_HIP_CHECK(hipMemcpyAsync(w.strand + q0 * k, dst, hits, hipMemcpyDeviceToHost, s), return false);
			}
		}
		if (w.rect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.rect + q0 * n, rf, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
		}
		if (w.vrect) {
			SA_HIP_CHECK(hipMemcpyAsync(w.vrect + q0 * n, vf, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, s), return false);
		}
		if (w.srect) {
			SA_HIP_CHECK(hipMemcpyAsync(h_bits.data(), stage.bits(), sizeof(uint64_t) * (size_t)nq * (size_t)words, hipMemcpyDeviceToHost, s), return false);
		}
		if (!stage.copy_denominators(q0) || !run.sync())
			return false;
		if (w.srect) /* the bitmap crossed the bus, one byte per cell is what the caller reads */
			for (int64_t r = 0; r < nq; r++)
				for (int64_t d = 0; d < n; d++)
					w.srect[(q0 + r) * n + d] = sa_strand_bit(h_bits.data() + r * words, n, (int32_t)d);
		return true;
	});
	if (!ok)
		return false;
	stage.publish_denominators();
	const PhaseClock &t = run.sy.clock;
	g_last_strands_seconds.store(t[SA_PH_FOLD] + t[SA_PH_STRAND_TAKE]);
	sa_search_quantity_last_set(t[SA_PH_QUANTITY]);
	/* (under percent identity the sweeps are the alignment as well: they are what delivers the scores) */
	sa_search_last_set(stage.aligned ? t[SA_PH_ALIGN] : t[SA_PH_QUANTITY], t[SA_PH_GATHER], t[SA_PH_SELECT], run.batches);
	return true;
}

} // namespace

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
		return sa_strand_fold_launch(d_vfwd, d_vrev, d_sfwd, d_srev, ctx->search_db, nq, d_vbest, d_sbest, d_bits, (hipStream_t)stream);
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
		return sa_hits_above_strand_launch(d_bits, ctx->search_db, nq, d_offsets, d_index, d_strand, (hipStream_t)stream);
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
