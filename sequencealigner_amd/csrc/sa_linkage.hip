/*
 * sa_linkage.hip -- the single-linkage tree of the finished device matrix: its maximum spanning tree under the contract's
 * total order, by Boruvka rounds over the device-resident packed triangle (sa_ctx_linkage, sa_hip_linkage, sa_zjob_linkage),
 * and the two host-only readers of a tree (sa_linkage_labels, sa_linkage_merges).  No reference counterpart: the reference
 * delivers the whole matrix and leaves the clustering to the host.
 *
 * A component is named by one of its vertices (comp[v]; at first comp[v] = v).  One round is five kernels in stream order; the
 * kernel boundaries are the only grid-wide barriers, no workgroup ever waits for another one:
 *   prepare  parent[v] = v, the per-component cells emptied; flag[round] = 1 iff some comp[v] differs from comp[0], i.e. more
 *            than one component is left.  Every later kernel of the round returns at once when the flag is 0.
 *   best     the sweep of sa_k_edges (sa_edges.hip), unchanged: a workgroup of four waves owns R = 16 rows and walks all N
 *            columns in blocks of R x 64, left of the diagonal read along c, right of it along r and turned in LDS, the next
 *            block's loads in flight while the current one is scanned.  Column c is a candidate of row r iff comp[c] != comp[r];
 *            a lane keeps the best candidate of its columns (ascending c is ascending packed index, so a later equal score
 *            never wins), the wave reduces (has, score, p) under sa_lk_before.  vscore[r] / vp[r] hold the result (vp = -1: no
 *            candidate -- never a score value), and the score goes into an integer atomic max of r's component.
 *   min      every vertex whose score equals its component's maximum: integer atomic min of its p.  Max, then min across a
 *            kernel boundary: neither depends on the order of arrival.
 *   hook     one thread per component C: the component D at the other end of C's pair becomes its parent, by the root rule
 *            (sa_lk_parent).  A C that is no longer a root stores its pair in slot C: a vertex stops being a root once, so the
 *            N slots take the N - 1 pairs without any counter.
 *   relabel  comp[v] = the root of comp[v]'s parent chain; the walk ends after N steps at the latest.
 * ceil(log2 N) rounds are enqueued (components at least halve per round), then
 *   sort     rank of a slot = the number of filled slots that come before it (N^2 comparisons through LDS tiles); the pair goes
 *            to place `rank`.  Where a round stored a pair has no influence on the result.
 * Every loop is bounded by N, every position and packed index is 64-bit.
 */
#include <atomic>
#include <new>

#include "sa_ctx.h"
#include "sa_linkage_core.h"

struct sa_linkage {
	int32_t num = 0;
	int32_t *pairs = nullptr; /* 2 (num - 1) (one element when num == 1: never a null pointer for a valid result) */
	int32_t *score = nullptr; /* num - 1 */
	~sa_linkage()
	{
		free(pairs);
		free(score);
	}
};

namespace {

constexpr int LK_THREADS = 256; /* four waves */
constexpr int R = 16;           /* rows of a workgroup; divides 64 (sa_neighbors.hip: why 16) */
constexpr int Q = R / 4;        /* rows per wave = elements of a block per thread */
constexpr int LK_FLAGS = 64;    /* one flag per round; ceil(log2 N) <= 31 */
constexpr unsigned long long LK_NONE = ~0ull; /* as int64_t: -1, no packed index */

/* the scratch memory of a call, carved up: 64-bit arrays first */
struct LkScratch {
	int32_t *flag;            /* LK_FLAGS: round k met more than one component */
	unsigned long long *cp;   /* N, by component: the smallest p among the vertices that hold the component's best score */
	int64_t *ep;              /* N, slot C: the pair C recorded when it stopped being a root, -1: none */
	int64_t *vp;              /* N, by vertex: packed index of its best candidate, -1: none */
	int32_t *comp, *parent;   /* N each */
	int32_t *vscore;          /* N, by vertex */
	uint32_t *cmax;           /* N, by component: the best score, sign bit flipped (unsigned order = signed order) */
	int32_t *es;              /* N, slot C: the score of ep */
};

constexpr size_t LK_PER_VERTEX = 3 * 8 + 5 * 4;

__host__ __device__ inline LkScratch lk_carve(void *scratch, int32_t num)
{
	LkScratch s;
	char *at = (char *)scratch;
	const size_t n = (size_t)num;
	s.flag = (int32_t *)at, at += LK_FLAGS * sizeof(int32_t);
	s.cp = (unsigned long long *)at, at += n * 8;
	s.ep = (int64_t *)at, at += n * 8;
	s.vp = (int64_t *)at, at += n * 8;
	s.comp = (int32_t *)at, at += n * 4;
	s.parent = (int32_t *)at, at += n * 4;
	s.vscore = (int32_t *)at, at += n * 4;
	s.cmax = (uint32_t *)at, at += n * 4;
	s.es = (int32_t *)at;
	return s;
}

__device__ __forceinline__ uint32_t lk_flip(int32_t score) { return (uint32_t)score ^ 0x80000000u; }

/* (the element layout of sa_k_edges) */
__device__ __forceinline__ int lk_row(bool along_r, int tid, int q) { return along_r ? tid % R : (tid >> 6) + 4 * q; }
__device__ __forceinline__ int lk_col(bool along_r, int tid, int q) { return along_r ? tid / R + (LK_THREADS / R) * q : tid & 63; }

__global__ __launch_bounds__(LK_THREADS) void sa_k_lk_prepare(void *scratch, int32_t num, int round)
{
	const LkScratch s = lk_carve(scratch, num);
	if (round > 0 && s.flag[round - 1] == 0)
		return;
	const int64_t v = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
	if (v >= num)
		return;
	int32_t mine = (int32_t)v, first = 0;
	if (round == 0) {
		s.comp[v] = mine;
		s.ep[v] = -1;
	} else {
		mine = s.comp[v];
		first = s.comp[0];
	}
	s.parent[v] = (int32_t)v;
	s.cmax[v] = 0u;
	s.cp[v] = LK_NONE;
	if (mine != first)
		s.flag[round] = 1; /* (every writer writes the same value) */
}

__global__ __launch_bounds__(LK_THREADS) void sa_k_lk_best(const int32_t *__restrict__ packed, int32_t num, void *scratch, int round)
{
	__shared__ int32_t turn[R][65];
	const LkScratch s = lk_carve(scratch, num);
	if (s.flag[round] == 0)
		return;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t r0 = (int64_t)blockIdx.x * R;
	const int blocks = (num + 63) / 64, diag = (int)(r0 / 64); /* (R divides 64: exactly one column block holds the diagonal) */

	int32_t comp_r[Q], best_s[Q], best_c[Q]; /* row r0 + wave + 4 q: its component (wave-uniform); this lane's best candidate */
	bool has[Q];
#pragma unroll
	for (int q = 0; q < Q; q++) {
		const int64_t r = r0 + wave + 4 * q;
		comp_r[q] = r < num ? s.comp[r] : -1;
		best_s[q] = 0;
		best_c[q] = 0;
		has[q] = false;
	}

	int32_t regs[Q], comp_next = -1;
	auto fetch = [&](int b) {
		const int64_t c0 = (int64_t)b * 64;
		const bool along_r = b > diag;
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const int64_t i = r0 + lk_row(along_r, tid, q), j = c0 + lk_col(along_r, tid, q);
			int32_t v = 0;
			if (i < num && j < num && i != j)
				v = packed[sa_lk_packed_at(i, j)];
			regs[q] = v;
		}
		comp_next = c0 + lane < num ? s.comp[c0 + lane] : -1; /* one coalesced load per wave and block */
	};

	fetch(0);
	for (int b = 0; b < blocks; b++) {
		const bool along_r = b > diag;
#pragma unroll
		for (int q = 0; q < Q; q++)
			turn[lk_row(along_r, tid, q)][lk_col(along_r, tid, q)] = regs[q];
		const int32_t comp_c = comp_next;
		__syncthreads();
		if (b + 1 < blocks)
			fetch(b + 1); /* in flight while this block is scanned */
		const int64_t c = (int64_t)b * 64 + lane;
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const int y = wave + 4 * q;
			const int64_t r = r0 + y;
			const int32_t v = turn[y][lane];
			/* ascending blocks are ascending p for this lane: only a strictly better score replaces the one it holds */
			if (r < num && c < num && c != r && comp_c != comp_r[q] && (!has[q] || v > best_s[q])) {
				has[q] = true;
				best_s[q] = v;
				best_c[q] = (int32_t)c;
			}
		}
		__syncthreads();
	}

#pragma unroll
	for (int q = 0; q < Q; q++) {
		const int64_t r = r0 + wave + 4 * q;
		if (r >= num) /* (wave-uniform) */
			continue;
		int h = has[q];
		int32_t sc = best_s[q];
		long long p = h ? (long long)sa_lk_packed_at(r, best_c[q]) : -1;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const int oh = __shfl_xor(h, d, 64);
			const int32_t os = __shfl_xor(sc, d, 64);
			const long long op = __shfl_xor(p, d, 64);
			if (oh && (!h || sa_lk_before(os, op, sc, p))) {
				h = 1;
				sc = os;
				p = op;
			}
		}
		if (lane == 0) {
			s.vscore[r] = sc;
			s.vp[r] = p;
			if (h)
				atomicMax(&s.cmax[comp_r[q]], lk_flip(sc));
		}
	}
}

__global__ __launch_bounds__(LK_THREADS) void sa_k_lk_min(void *scratch, int32_t num, int round)
{
	const LkScratch s = lk_carve(scratch, num);
	if (s.flag[round] == 0)
		return;
	const int64_t v = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
	if (v >= num)
		return;
	const int64_t p = s.vp[v];
	const int32_t c = s.comp[v];
	if (p >= 0 && lk_flip(s.vscore[v]) == s.cmax[c])
		atomicMin(&s.cp[c], (unsigned long long)p);
}

__global__ __launch_bounds__(LK_THREADS) void sa_k_lk_hook(void *scratch, int32_t num, int round)
{
	const LkScratch s = lk_carve(scratch, num);
	if (s.flag[round] == 0)
		return;
	const int64_t v = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
	if (v >= num)
		return;
	const int32_t c = (int32_t)v;
	if (s.comp[c] != c) /* (one thread per component: its root) */
		return;
	const int64_t pc = (int64_t)s.cp[c];
	if (pc < 0)
		return;
	int64_t lo, hi;
	sa_lk_unpack(pc, &lo, &hi);
	if (hi >= num)
		return;
	const int32_t a = s.comp[lo], b = s.comp[hi];
	if ((a == c) == (b == c)) /* (exactly one end is in c) */
		return;
	const int32_t d = a == c ? b : a;
	const int32_t up = sa_lk_parent(c, d, pc, (int64_t)s.cp[d]);
	s.parent[c] = up;
	if (up != c) {
		s.ep[c] = pc;
		s.es[c] = (int32_t)(s.cmax[c] ^ 0x80000000u);
	}
}

__global__ __launch_bounds__(LK_THREADS) void sa_k_lk_relabel(void *scratch, int32_t num, int round)
{
	const LkScratch s = lk_carve(scratch, num);
	if (s.flag[round] == 0)
		return;
	const int64_t v = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
	if (v >= num)
		return;
	int32_t c = s.comp[v];
	for (int32_t step = 0; step < num; step++) {
		const int32_t up = s.parent[c];
		if (up == c)
			break;
		c = up;
	}
	s.comp[v] = c;
}

__global__ __launch_bounds__(LK_THREADS) void sa_k_lk_sort(const void *scratch, int32_t num, int32_t *__restrict__ pairs,
							   int32_t *__restrict__ score)
{
	__shared__ int64_t tile_p[LK_THREADS];
	__shared__ int32_t tile_s[LK_THREADS];
	const LkScratch s = lk_carve(const_cast<void *>(scratch), num);
	const int tid = threadIdx.x;
	const int64_t v = (int64_t)blockIdx.x * LK_THREADS + tid;
	const int64_t pv = v < num ? s.ep[v] : -1;
	const int32_t sv = pv >= 0 ? s.es[v] : 0;
	int64_t rank = 0;
	for (int64_t base = 0; base < num; base += LK_THREADS) {
		const int64_t u = base + tid;
		const int64_t pu = u < num ? s.ep[u] : -1;
		tile_p[tid] = pu;
		tile_s[tid] = pu >= 0 ? s.es[u] : 0;
		__syncthreads();
#pragma unroll 8
		for (int t = 0; t < LK_THREADS; t++) {
			const int64_t pt = tile_p[t];
			rank += pt >= 0 && sa_lk_before(tile_s[t], pt, sv, pv);
		}
		__syncthreads();
	}
	if (pv >= 0 && rank < (int64_t)num - 1) {
		int64_t lo, hi;
		sa_lk_unpack(pv, &lo, &hi);
		pairs[2 * rank] = (int32_t)lo;
		pairs[2 * rank + 1] = (int32_t)hi;
		score[rank] = sv;
	}
}

std::atomic<double> g_last_linkage_seconds{ 0.0 };
std::atomic<int> g_last_linkage_rounds{ 0 };

int lk_rounds(int32_t num)
{
	int rounds = 0;
	while (((int64_t)1 << rounds) < num)
		rounds++;
	return rounds;
}

size_t lk_scratch_bytes(int32_t num) { return num < 1 ? 0 : LK_FLAGS * sizeof(int32_t) + LK_PER_VERTEX * (size_t)num; }

/* num >= 2; everything in order on `s` */
hipError_t launch_linkage(const int32_t *packed, int32_t num, int32_t *pairs, int32_t *score, void *scratch, hipStream_t s)
{
	const dim3 per_vertex((unsigned)((num + LK_THREADS - 1) / LK_THREADS)), per_rows((unsigned)((num + R - 1) / R)), threads(LK_THREADS);
	if (hipError_t e = hipMemsetAsync(scratch, 0, LK_FLAGS * sizeof(int32_t), s); e != hipSuccess)
		return e;
	const int rounds = lk_rounds(num);
	for (int k = 0; k < rounds; k++) {
		hipLaunchKernelGGL(sa_k_lk_prepare, per_vertex, threads, 0, s, scratch, num, k);
		hipLaunchKernelGGL(sa_k_lk_best, per_rows, threads, 0, s, packed, num, scratch, k);
		hipLaunchKernelGGL(sa_k_lk_min, per_vertex, threads, 0, s, scratch, num, k);
		hipLaunchKernelGGL(sa_k_lk_hook, per_vertex, threads, 0, s, scratch, num, k);
		hipLaunchKernelGGL(sa_k_lk_relabel, per_vertex, threads, 0, s, scratch, num, k);
		if (hipError_t e = hipGetLastError(); e != hipSuccess)
			return e;
	}
	hipLaunchKernelGGL(sa_k_lk_sort, per_vertex, threads, 0, s, (const void *)scratch, num, pairs, score);
	return hipGetLastError();
}

const char *lk_message(int code)
{
	switch (code) {
	case SA_LK_RANGE:
		return "not a tree: an index is out of range";
	case SA_LK_LO_HI:
		return "not a tree: a pair does not have lo < hi";
	case SA_LK_CYCLE:
		return "not a tree: the pairs close a cycle";
	case SA_LK_ORDER:
		return "the scores are not in the order of the contract";
	default:
		return "out of host memory";
	}
}

} // namespace

/* The tree of a finished device matrix into HOST arrays, in order on `s`: what sa_hip_linkage and sa_zjob_linkage share.  The
 * current device is the matrix's.  Leaves the device time of rounds + sort for sa_hip_last_linkage_seconds and the number of
 * rounds for sa_hip_last_linkage_rounds.  nullptr + sa_set_error on failure. */
sa_linkage *sa_linkage_to_host(const char *who, const int32_t *d_packed, int32_t num, hipStream_t s)
{
	struct Tmp {
		int32_t *d_out = nullptr;
		void *d_scratch = nullptr;
		hipEvent_t e[2] = { nullptr, nullptr };
		sa_linkage *res = nullptr;
		~Tmp()
		{
			(void)hipFree(d_out);
			(void)hipFree(d_scratch);
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
	const size_t merges = (size_t)num - 1, room = merges ? merges : 1;
	t.res = new sa_linkage;
	t.res->num = num;
	t.res->pairs = (int32_t *)malloc(2 * room * sizeof(int32_t));
	t.res->score = (int32_t *)malloc(room * sizeof(int32_t));
	if (!t.res->pairs || !t.res->score) {
		sa_set_error("%s: out of host memory for the tree of %d sequences", who, num);
		return nullptr;
	}
	float ms = 0.f;
	int rounds = 0;
	if (merges) {
		int32_t flags[LK_FLAGS];
		SA_HIP_CHECK(hipMalloc(&t.d_out, 3 * merges * sizeof(int32_t)), return nullptr);
		SA_HIP_CHECK(hipMalloc(&t.d_scratch, lk_scratch_bytes(num)), return nullptr);
		for (hipEvent_t &ev : t.e)
			SA_HIP_CHECK(hipEventCreate(&ev), return nullptr);
		SA_HIP_CHECK(hipEventRecord(t.e[0], s), return nullptr);
		SA_HIP_CHECK(launch_linkage(d_packed, num, t.d_out, t.d_out + 2 * merges, t.d_scratch, s), return nullptr);
		SA_HIP_CHECK(hipEventRecord(t.e[1], s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(t.res->pairs, t.d_out, 2 * merges * sizeof(int32_t), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(t.res->score, t.d_out + 2 * merges, merges * sizeof(int32_t), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(flags, t.d_scratch, sizeof(flags), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipStreamSynchronize(s), return nullptr);
		SA_HIP_CHECK(hipEventElapsedTime(&ms, t.e[0], t.e[1]), return nullptr);
		for (int32_t f : flags)
			rounds += f != 0;
	}
	g_last_linkage_seconds.store((double)ms * 1e-3);
	g_last_linkage_rounds.store(rounds);
	sa_linkage *res = t.res;
	t.res = nullptr;
	return res;
}

extern "C" size_t sa_linkage_scratch_bytes(int32_t num) { return lk_scratch_bytes(num); }

extern "C" int sa_ctx_linkage(sa_ctx *ctx, const int32_t *d_packed, int32_t *d_pairs, int32_t *d_score, void *d_scratch, void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_linkage"))
		return 1;
	return sa_guard("sa_ctx_linkage", 1, [&] {
		if (!ctx || !d_packed || !d_pairs || !d_score || !d_scratch) {
			sa_set_error("sa_ctx_linkage: null argument");
			return 1;
		}
		if ((uintptr_t)d_scratch % 8) {
			sa_set_error("sa_ctx_linkage: the scratch memory is not aligned to 8 bytes");
			return 1;
		}
		if (ctx->num < 2) /* (no pair, no merge) */
			return 0;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_linkage(d_packed, ctx->num, d_pairs, d_score, d_scratch, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" const int32_t *sa_linkage_pairs(const sa_linkage *l, int32_t *merges)
{
	return sa_guard("sa_linkage_pairs", (const int32_t *)nullptr, [&] {
		if (merges)
			*merges = l ? l->num - 1 : 0;
		return l ? (const int32_t *)l->pairs : nullptr;
	});
}

extern "C" const int32_t *sa_linkage_score(const sa_linkage *l)
{
	return sa_guard("sa_linkage_score", (const int32_t *)nullptr, [&] { return l ? (const int32_t *)l->score : nullptr; });
}

extern "C" void sa_linkage_destroy(sa_linkage *l)
{
	sa_guard_void("sa_linkage_destroy", [&] { delete l; });
}

extern "C" double sa_hip_last_linkage_seconds(void)
{
	return sa_guard("sa_hip_last_linkage_seconds", 0.0, [&] { return g_last_linkage_seconds.load(); });
}

extern "C" int sa_hip_last_linkage_rounds(void)
{
	return sa_guard("sa_hip_last_linkage_rounds", 0, [&] { return g_last_linkage_rounds.load(); });
}

/* ---- host only: a tree's readers ------------------------------------------------------------------------------------------ */
extern "C" int32_t sa_linkage_labels(const int32_t *pairs, const int32_t *score, int32_t num, int32_t min_score, int32_t *labels)
{
	return sa_guard("sa_linkage_labels", (int32_t)-1, [&]() -> int32_t {
		if (!labels || (num > 1 && (!pairs || !score))) {
			sa_set_error("sa_linkage_labels: null argument");
			return -1;
		}
		if (num < 1) {
			sa_set_error("sa_linkage_labels: %d sequences", num);
			return -1;
		}
		const int32_t clusters = sa_lk_labels(pairs, score, num, min_score, labels);
		if (clusters < 0)
			sa_set_error("sa_linkage_labels: %s", lk_message(clusters));
		return clusters < 0 ? -1 : clusters;
	});
}

extern "C" int sa_linkage_merges(const int32_t *pairs, int32_t num, int32_t *left, int32_t *right, int32_t *size)
{
	return sa_guard("sa_linkage_merges", 1, [&] {
		if (num > 1 && (!pairs || !left || !right || !size)) {
			sa_set_error("sa_linkage_merges: null argument");
			return 1;
		}
		if (num < 1) {
			sa_set_error("sa_linkage_merges: %d sequences", num);
			return 1;
		}
		const int bad = sa_lk_merges(pairs, num, left, right, size);
		if (bad)
			sa_set_error("sa_linkage_merges: %s", lk_message(bad));
		return bad ? 1 : 0;
	});
}
