/*
 * sa_agglo.hip -- complete and average linkage (UPGMA) of the finished device matrix: the greedy agglomeration under the
 * contract's total order over a square working copy of the device-resident packed triangle (sa_ctx_agglomerate,
 * sa_hip_agglomerate, sa_zjob_agglomerate), and the host-only reader of such a tree (sa_agglo_labels).  No reference
 * counterpart: the reference delivers the whole matrix and leaves the clustering to the host.
 *
 * Working state, all of it in the caller's scratch memory (ag_carve):
 *   W       N x N, symmetric: the similarity of the clusters named r and c -- int32 minima (complete) or int64 sums (average).
 *           Rows are contiguous, which every scan wants; rows and columns of clusters that were merged away are never read.
 *   size    members of cluster c;  active  1 while c names a cluster
 *   best    the partner of c that comes first in the order among the active clusters other than c;  bsim  W[c][best[c]]
 *   cell    the pair (a, b) the step merges;  count  the row rescans (a diagnostic)
 * Kernels, in stream order; the kernel boundaries are the only grid-wide barriers, no workgroup ever waits for another one:
 *   expand  W from the packed triangle, a 64 x 64 tile per workgroup: the tile below the diagonal is read along its rows,
 *           written as it is and, turned in LDS, as its mirror image; size = 1, active = 1, count = 0
 *   scan    a wave per row: lanes stride the row and keep the first candidate of their columns (ascending column is ascending
 *           packed index, so a later equal similarity never wins), the wave reduces under sa_ag_before
 *   pick    one workgroup, step t: the first (c, best[c]) over the active rows is the merge (a, b); pairs, score, the cell;
 *           size[a] += size[b], active[b] = 0
 *   merge   step t.  Workgroup 0 owns row a: W[a][c] = combine(W[a][c], W[b][c]) over the active c and, in the same pass, the
 *           new best[a].  In every other workgroup a wave owns a row c: W[c][a] = combine(W[c][a], W[c][b]), then the cache rule
 *           (sa_ag_cache); only a row whose cached partner was a or b and whose new entry comes after the cached key is scanned
 *           again, and counted.  Row a reads row b, which nobody writes; row c reads and writes row c alone: the two halves of
 *           the symmetric update never meet.  A value a wave has just computed is used from its register, never read back.
 * The scans are bound by memory latency, not bandwidth (one wave walks a row of N), so a trip of a scan issues the loads of
 * AG_SCAN_U columns per lane (AG_ROW_U in row a's pass, AG_PICK_U rows per thread in pick) before it tests the first of them.
 * 2 + 2 (N - 1) launches are enqueued with no host synchronisation; the step number travels as a kernel argument.  Every loop
 * is bounded by N, every matrix position is 64-bit, the rescan count is the only atomic.
 */
#include <atomic>
#include <new>

#include "sa_agglo_core.h"
#include "sa_ctx.h"

/* (sa_linkage.hip's result object: the same definition, so that sa_linkage_pairs / _score / _destroy serve both trees) */
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

constexpr int AG_THREADS = 256;                /* four waves */
constexpr int AG_WAVES = AG_THREADS / 64;      /* rows of a merge / scan workgroup */
constexpr int AG_PICK_THREADS = 1024;          /* the one workgroup of pick */
constexpr int AG_PICK_WAVES = AG_PICK_THREADS / 64;
constexpr int AG_TILE = 64;                    /* expand */
constexpr int AG_SCAN_U = 16;                  /* columns per lane and trip of a row scan: loads in flight (latency-bound otherwise) */
constexpr int AG_ROW_U = 8;                    /* ... of row a's pass, two matrix loads each */
constexpr int AG_PICK_U = 4;                   /* rows per thread and trip of pick */
constexpr size_t AG_HEAD = 64;                 /* bytes: count (8), cell (2 x 4), room */

template <int M> struct AgState {
	typedef typename sa_ag_rule<M>::T T;
	unsigned long long *count;
	int32_t *cell;
	T *w, *bsim;
	int32_t *size, *active, *best;
};

template <int M> __host__ __device__ inline AgState<M> ag_carve(void *scratch, int32_t num)
{
	typedef typename sa_ag_rule<M>::T T;
	AgState<M> s;
	char *at = (char *)scratch;
	const size_t n = (size_t)num;
	s.count = (unsigned long long *)at;
	s.cell = (int32_t *)(at + 8), at += AG_HEAD;
	s.w = (T *)at, at += n * n * sizeof(T);
	s.bsim = (T *)at, at += n * sizeof(T);
	s.size = (int32_t *)at, at += n * 4;
	s.active = (int32_t *)at, at += n * 4;
	s.best = (int32_t *)at;
	return s;
}

size_t ag_scratch_bytes(int32_t num, int32_t method)
{
	if (num < 2 || (method != SA_AGGLO_COMPLETE && method != SA_AGGLO_AVERAGE))
		return 0;
	if (num > (method == SA_AGGLO_AVERAGE ? SA_AGGLO_AVERAGE_MAX_NUM : SA_AGGLO_COMPLETE_MAX_NUM))
		return 0;
	const size_t n = (size_t)num, t = method == SA_AGGLO_AVERAGE ? 8 : 4;
	return AG_HEAD + t * (n * n + n) + 12 * n;
}

__device__ __forceinline__ int32_t ag_shfl(int32_t v, int d) { return __shfl_xor(v, d, 64); }
__device__ __forceinline__ int64_t ag_shfl(int64_t v, int d) { return (int64_t)__shfl_xor((long long)v, d, 64); }

/* a candidate: similarity s / n at packed index p; h = 0: none yet (never a similarity value).  (No initialisers: it lives in
 * LDS as well; ag_none is the empty one.) */
template <int M> struct AgCand {
	typename sa_ag_rule<M>::T s;
	int64_t n, p;
	int h;
	__device__ __forceinline__ void take_if_first(const AgCand &o)
	{
		if (o.h && (!h || sa_ag_before<M>(o.s, o.n, o.p, s, n, p)))
			*this = o;
	}
};

template <int M> __device__ __forceinline__ AgCand<M> ag_none()
{
	AgCand<M> c;
	c.s = 0;
	c.n = 1;
	c.p = 0;
	c.h = 0;
	return c;
}

/* every lane gets the first candidate of the wave */
template <int M> __device__ __forceinline__ void ag_wave_first(AgCand<M> &c)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		AgCand<M> o;
		o.h = ag_shfl((int32_t)c.h, d);
		o.s = ag_shfl(c.s, d);
		o.n = M == SA_AGGLO_AVERAGE ? ag_shfl(c.n, d) : 1; /* (complete linkage does not read n) */
		o.p = ag_shfl(c.p, d);
		c.take_if_first(o);
	}
}

/* the partner of row c behind a packed index of that row */
__device__ __forceinline__ int32_t ag_partner(int64_t p, int32_t c)
{
	int64_t lo, hi;
	sa_lk_unpack(p, &lo, &hi);
	return (int32_t)(lo == c ? hi : lo);
}

/* one wave: the first candidate of row c among the active d != c; `a` (or -1) is a column whose value `wa` is in a register */
template <int M>
__device__ __forceinline__ AgCand<M> ag_scan_row(const AgState<M> &s, int32_t num, int32_t c, int lane, int32_t a,
						 typename sa_ag_rule<M>::T wa)
{
	typedef typename sa_ag_rule<M>::T T;
	const T *row = s.w + sa_ag_at(c, 0, num);
	AgCand<M> mine = ag_none<M>();
	int32_t at = 0;
	/* a trip is AG_SCAN_U loads per array, all in flight at once: they do not wait for what the candidate test decides.  A column
	 * past the row is read at the row's last one (in bounds) and not used. */
	for (int32_t d0 = 0; d0 < num; d0 += 64 * AG_SCAN_U) {
		T v[AG_SCAN_U];
		int32_t members[AG_SCAN_U], act[AG_SCAN_U];
#pragma unroll
		for (int u = 0; u < AG_SCAN_U; u++) {
			const int32_t d = d0 + 64 * u + lane, at_most = d < num ? d : num - 1;
			act[u] = s.active[at_most];
			members[u] = s.size[at_most];
			v[u] = row[at_most];
		}
#pragma unroll
		for (int u = 0; u < AG_SCAN_U; u++) { /* (ascending u is ascending d for this lane) */
			const int32_t d = d0 + 64 * u + lane;
			if (d < num && d != c && act[u]) {
				const T x = d == a ? wa : v[u];
				const int64_t n = members[u];
				if (!mine.h || sa_ag_rule<M>::cmp(x, n, mine.s, mine.n) > 0) { /* (ascending d is ascending p) */
					mine.h = 1;
					mine.s = x;
					mine.n = n;
					at = d;
				}
			}
		}
	}
	mine.p = mine.h ? sa_lk_packed_at(c, at) : 0;
	ag_wave_first<M>(mine);
	return mine;
}

template <int M> __global__ __launch_bounds__(AG_THREADS) void sa_k_ag_expand(const int32_t *__restrict__ packed, int32_t num, void *scratch)
{
	typedef typename sa_ag_rule<M>::T T;
	__shared__ int32_t turn[AG_TILE][AG_TILE + 1];
	if (blockIdx.x > blockIdx.y) /* (tiles on and below the diagonal) */
		return;
	const AgState<M> s = ag_carve<M>(scratch, num);
	const int tid = threadIdx.x, x = tid & 63, y0 = tid >> 6;
	const int64_t r0 = (int64_t)blockIdx.y * AG_TILE, c0 = (int64_t)blockIdx.x * AG_TILE;
	for (int y = y0; y < AG_TILE; y += AG_WAVES) {
		const int64_t r = r0 + y, c = c0 + x;
		int32_t v = 0;
		if (r < num && c < r) {
			v = packed[r * (r - 1) / 2 + c];
			s.w[sa_ag_at(r, c, num)] = (T)v;
		}
		turn[y][x] = v;
	}
	__syncthreads();
	for (int y = y0; y < AG_TILE; y += AG_WAVES) {
		const int64_t r = c0 + y, c = r0 + x; /* the mirror image: row from the tile's columns */
		if (c < num && r < c)
			s.w[sa_ag_at(r, c, num)] = (T)turn[x][y];
	}
	if (blockIdx.x == blockIdx.y && tid < AG_TILE) {
		const int64_t r = r0 + tid;
		if (r < num) {
			s.w[sa_ag_at(r, r, num)] = 0; /* (never read as a pair) */
			s.size[r] = 1;
			s.active[r] = 1;
		}
		if (r == 0) {
			*s.count = 0;
			s.cell[0] = s.cell[1] = -1;
		}
	}
}

template <int M> __global__ __launch_bounds__(AG_THREADS) void sa_k_ag_scan(int32_t num, void *scratch)
{
	const AgState<M> s = ag_carve<M>(scratch, num);
	const int lane = threadIdx.x & 63;
	const int64_t r = (int64_t)blockIdx.x * AG_WAVES + (threadIdx.x >> 6);
	if (r >= num) /* (wave-uniform) */
		return;
	const int32_t c = (int32_t)r;
	const AgCand<M> first = ag_scan_row<M>(s, num, c, lane, -1, 0);
	if (lane == 0) {
		s.best[c] = first.h ? ag_partner(first.p, c) : -1;
		s.bsim[c] = first.s;
	}
}

template <int M>
__global__ __launch_bounds__(AG_PICK_THREADS) void sa_k_ag_pick(int32_t num, void *scratch, int32_t step, int32_t *__restrict__ pairs,
							      int32_t *__restrict__ score)
{
	__shared__ AgCand<M> part[AG_PICK_WAVES];
	const AgState<M> s = ag_carve<M>(scratch, num);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	AgCand<M> mine = ag_none<M>();
	/* two levels of loads per trip, each AG_PICK_U wide and issued together: the row's cache, then its partner's size.  A row past
	 * N is read at row N - 1, a partner outside [0, N) at 0 (both in bounds), and not used. */
	for (int32_t c0 = 0; c0 < num; c0 += AG_PICK_THREADS * AG_PICK_U) {
		typename sa_ag_rule<M>::T sim[AG_PICK_U];
		int32_t partner[AG_PICK_U], members[AG_PICK_U], act[AG_PICK_U], partner_members[AG_PICK_U], partner_act[AG_PICK_U];
#pragma unroll
		for (int u = 0; u < AG_PICK_U; u++) {
			const int32_t c = c0 + AG_PICK_THREADS * u + tid, at_most = c < num ? c : num - 1;
			act[u] = s.active[at_most];
			partner[u] = s.best[at_most];
			sim[u] = s.bsim[at_most];
			members[u] = s.size[at_most];
		}
#pragma unroll
		for (int u = 0; u < AG_PICK_U; u++) {
			const int32_t d = partner[u] >= 0 && partner[u] < num ? partner[u] : 0;
			partner_members[u] = s.size[d];
			partner_act[u] = s.active[d];
		}
#pragma unroll
		for (int u = 0; u < AG_PICK_U; u++) {
			const int32_t c = c0 + AG_PICK_THREADS * u + tid, d = partner[u];
			if (c >= num || !act[u] || d < 0 || d >= num || d == c || !partner_act[u])
				continue;
			AgCand<M> o;
			o.h = 1;
			o.s = sim[u];
			o.n = (int64_t)members[u] * partner_members[u];
			o.p = sa_lk_packed_at(c, d);
			mine.take_if_first(o);
		}
	}
	ag_wave_first<M>(mine);
	if (lane == 0)
		part[wave] = mine;
	__syncthreads(); /* (also: every read of size / active above is behind us) */
	if (tid != 0)
		return;
	for (int w = 1; w < AG_PICK_WAVES; w++)
		mine.take_if_first(part[w]);
	int64_t lo = -1, hi = -1;
	if (mine.h)
		sa_lk_unpack(mine.p, &lo, &hi);
	if (!mine.h || hi >= num) { /* (cannot happen while two clusters are active; the step then merges nothing) */
		s.cell[0] = s.cell[1] = -1;
		pairs[2 * (int64_t)step] = pairs[2 * (int64_t)step + 1] = 0;
		score[step] = 0;
		return;
	}
	s.cell[0] = (int32_t)lo;
	s.cell[1] = (int32_t)hi;
	pairs[2 * (int64_t)step] = (int32_t)lo;
	pairs[2 * (int64_t)step + 1] = (int32_t)hi;
	score[step] = sa_ag_rule<M>::score(mine.s, mine.n);
	s.size[lo] += s.size[hi];
	s.active[hi] = 0;
}

template <int M> __global__ __launch_bounds__(AG_THREADS) void sa_k_ag_merge(int32_t num, void *scratch)
{
	typedef typename sa_ag_rule<M>::T T;
	__shared__ AgCand<M> part[AG_WAVES];
	const AgState<M> s = ag_carve<M>(scratch, num);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int32_t a = s.cell[0], b = s.cell[1];
	if (a < 0 || b <= a || b >= num) /* (uniform over the grid) */
		return;

	if (blockIdx.x == 0) { /* row a, the whole workgroup */
		T *row_a = s.w + sa_ag_at(a, 0, num);
		const T *row_b = s.w + sa_ag_at(b, 0, num);
		AgCand<M> mine = ag_none<M>();
		int32_t at = 0;
		for (int32_t d0 = 0; d0 < num; d0 += AG_THREADS * AG_ROW_U) { /* (the loads of a trip in flight together, as in ag_scan_row) */
			T va[AG_ROW_U], vb[AG_ROW_U];
			int32_t members[AG_ROW_U], act[AG_ROW_U];
#pragma unroll
			for (int u = 0; u < AG_ROW_U; u++) {
				const int32_t d = d0 + AG_THREADS * u + tid, at_most = d < num ? d : num - 1;
				act[u] = s.active[at_most];
				members[u] = s.size[at_most];
				va[u] = row_a[at_most];
				vb[u] = row_b[at_most];
			}
#pragma unroll
			for (int u = 0; u < AG_ROW_U; u++) { /* (ascending u is ascending d for this thread) */
				const int32_t d = d0 + AG_THREADS * u + tid;
				if (d < num && d != a && act[u]) { /* (b is not active any more) */
					const T v = sa_ag_rule<M>::combine(va[u], vb[u]);
					row_a[d] = v;
					const int64_t n = members[u];
					if (!mine.h || sa_ag_rule<M>::cmp(v, n, mine.s, mine.n) > 0) {
						mine.h = 1;
						mine.s = v;
						mine.n = n;
						at = d;
					}
				}
			}
		}
		mine.p = mine.h ? sa_lk_packed_at(a, at) : 0;
		ag_wave_first<M>(mine);
		if (lane == 0)
			part[wave] = mine;
		__syncthreads();
		if (tid == 0) {
			for (int w = 1; w < AG_WAVES; w++)
				mine.take_if_first(part[w]);
			s.best[a] = mine.h ? ag_partner(mine.p, a) : -1; /* (none: a is the last cluster) */
			s.bsim[a] = mine.s;
		}
		return;
	}

	const int64_t r = (int64_t)(blockIdx.x - 1) * AG_WAVES + wave;
	if (r >= num) /* (wave-uniform, as everything below) */
		return;
	const int32_t c = (int32_t)r;
	if (c == a || !s.active[c])
		return;
	const int64_t ca = sa_ag_at(c, a, num);
	const T v = sa_ag_rule<M>::combine(s.w[ca], s.w[sa_ag_at(c, b, num)]);
	const int32_t old = s.best[c];
	int what = SA_AG_RESCAN;
	if (old >= 0 && old < num && old != c)
		what = sa_ag_cache<M>(c, a, b, old, s.bsim[c], sa_ag_size_before(s.size, old, a, b), v, s.size[a]);
	if (what == SA_AG_RESCAN) {
		const AgCand<M> first = ag_scan_row<M>(s, num, c, lane, a, v);
		if (lane == 0) {
			s.w[ca] = v;
			s.best[c] = first.h ? ag_partner(first.p, c) : -1;
			s.bsim[c] = first.s;
			atomicAdd(s.count, 1ull);
		}
	} else if (lane == 0) {
		s.w[ca] = v;
		if (what == SA_AG_TAKE) {
			s.best[c] = a;
			s.bsim[c] = v;
		}
	}
}

std::atomic<double> g_last_agglo_seconds{ 0.0 };
std::atomic<int64_t> g_last_agglo_rescans{ 0 };

/* num >= 2, method and num checked; everything in order on `st` */
template <int M> hipError_t launch_agglo_t(const int32_t *packed, int32_t num, int32_t *pairs, int32_t *score, void *scratch, hipStream_t st)
{
	const unsigned tiles = (unsigned)((num + AG_TILE - 1) / AG_TILE), rows = (unsigned)((num + AG_WAVES - 1) / AG_WAVES);
	hipLaunchKernelGGL(sa_k_ag_expand<M>, dim3(tiles, tiles), dim3(AG_THREADS), 0, st, packed, num, scratch);
	hipLaunchKernelGGL(sa_k_ag_scan<M>, dim3(rows), dim3(AG_THREADS), 0, st, num, scratch);
	if (hipError_t e = hipGetLastError(); e != hipSuccess)
		return e;
	for (int32_t t = 0; t + 1 < num; t++) {
		hipLaunchKernelGGL(sa_k_ag_pick<M>, dim3(1), dim3(AG_PICK_THREADS), 0, st, num, scratch, t, pairs, score);
		hipLaunchKernelGGL(sa_k_ag_merge<M>, dim3(rows + 1), dim3(AG_THREADS), 0, st, num, scratch);
		if (hipError_t e = hipGetLastError(); e != hipSuccess)
			return e;
	}
	return hipSuccess;
}

hipError_t launch_agglo(const int32_t *packed, int32_t num, int32_t method, int32_t *pairs, int32_t *score, void *scratch, hipStream_t st)
{
	return method == SA_AGGLO_AVERAGE ? launch_agglo_t<SA_AGGLO_AVERAGE>(packed, num, pairs, score, scratch, st)
					  : launch_agglo_t<SA_AGGLO_COMPLETE>(packed, num, pairs, score, scratch, st);
}

const char *ag_message(int code)
{
	switch (code) {
	case SA_LK_RANGE:
		return "not a tree: an index is out of range";
	case SA_LK_LO_HI:
		return "not a tree: a pair does not have lo < hi";
	case SA_LK_CYCLE:
		return "not a tree: the pairs close a cycle";
	case SA_AG_NOT_DESCENDING:
		return "the scores increase: not the merges of an agglomeration";
	default:
		return "out of host memory";
	}
}

} // namespace

/* method and N, before anything is launched or a device is looked for */
bool sa_agglo_check(const char *who, int32_t num, int32_t method)
{
	if (method == SA_AGGLO_SINGLE) {
		sa_set_error("%s: method 0 is single linkage, which sa_ctx_linkage / sa_hip_linkage / sa_zjob_linkage build", who);
		return false;
	}
	if (method != SA_AGGLO_COMPLETE && method != SA_AGGLO_AVERAGE) {
		sa_set_error("%s: method %d is neither SA_AGGLO_COMPLETE (1) nor SA_AGGLO_AVERAGE (2)", who, method);
		return false;
	}
	if (num < 1) {
		sa_set_error("%s: %d sequences", who, num);
		return false;
	}
	if (method == SA_AGGLO_AVERAGE && num > SA_AGGLO_AVERAGE_MAX_NUM) {
		sa_set_error("%s: average linkage of %d sequences: the int64 sums hold at most %d", who, num, SA_AGGLO_AVERAGE_MAX_NUM);
		return false;
	}
	if (num > SA_AGGLO_COMPLETE_MAX_NUM) {
		sa_set_error("%s: %d sequences: the working matrix holds at most %d", who, num, SA_AGGLO_COMPLETE_MAX_NUM);
		return false;
	}
	return true;
}

/* The tree of a finished device matrix into HOST arrays, in order on `s`: what sa_hip_agglomerate and sa_zjob_agglomerate
 * share.  The current device is the matrix's.  Leaves the device time for sa_hip_last_agglomerate_seconds and the row rescans
 * for sa_hip_last_agglomerate_rescans.  nullptr + sa_set_error on failure. */
sa_linkage *sa_agglomerate_to_host(const char *who, const int32_t *d_packed, int32_t num, int32_t method, hipStream_t s)
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
	if (!sa_agglo_check(who, num, method))
		return nullptr;
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
	unsigned long long rescans = 0;
	if (merges) {
		const size_t bytes = ag_scratch_bytes(num, method);
		SA_HIP_CHECK(hipMalloc(&t.d_out, 3 * merges * sizeof(int32_t)), return nullptr);
		if (hipMalloc(&t.d_scratch, bytes) != hipSuccess) {
			(void)hipGetLastError();
			t.d_scratch = nullptr;
			sa_set_error("%s: the working matrix of %d sequences (%zu bytes, %.2f GiB) does not fit the device's memory beside the packed matrix",
				     who, num, bytes, (double)bytes / (double)(1 << 30));
			return nullptr;
		}
		for (hipEvent_t &ev : t.e)
			SA_HIP_CHECK(hipEventCreate(&ev), return nullptr);
		SA_HIP_CHECK(hipEventRecord(t.e[0], s), return nullptr);
		SA_HIP_CHECK(launch_agglo(d_packed, num, method, t.d_out, t.d_out + 2 * merges, t.d_scratch, s), return nullptr);
		SA_HIP_CHECK(hipEventRecord(t.e[1], s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(t.res->pairs, t.d_out, 2 * merges * sizeof(int32_t), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(t.res->score, t.d_out + 2 * merges, merges * sizeof(int32_t), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipMemcpyAsync(&rescans, t.d_scratch, sizeof(rescans), hipMemcpyDeviceToHost, s), return nullptr);
		SA_HIP_CHECK(hipStreamSynchronize(s), return nullptr);
		SA_HIP_CHECK(hipEventElapsedTime(&ms, t.e[0], t.e[1]), return nullptr);
	}
	g_last_agglo_seconds.store((double)ms * 1e-3);
	g_last_agglo_rescans.store((int64_t)rescans);
	sa_linkage *res = t.res;
	t.res = nullptr;
	return res;
}

extern "C" size_t sa_agglo_scratch_bytes(int32_t num, int32_t method) { return ag_scratch_bytes(num, method); }

extern "C" int sa_ctx_agglomerate(sa_ctx *ctx, const int32_t *d_packed, int32_t method, int32_t *d_pairs, int32_t *d_score, void *d_scratch,
				  void *stream)
{
	if (sa_search_refused(ctx, "sa_ctx_agglomerate"))
		return 1;
	return sa_guard("sa_ctx_agglomerate", 1, [&] {
		if (!ctx || !d_packed || !d_pairs || !d_score || !d_scratch) {
			sa_set_error("sa_ctx_agglomerate: null argument");
			return 1;
		}
		if (!sa_agglo_check("sa_ctx_agglomerate", ctx->num, method))
			return 1;
		if ((uintptr_t)d_scratch % 8) {
			sa_set_error("sa_ctx_agglomerate: the scratch memory is not aligned to 8 bytes");
			return 1;
		}
		if (ctx->num < 2) /* (no pair, no merge) */
			return 0;
		SA_HIP_CHECK(hipSetDevice(ctx->device), return 1);
		SA_HIP_CHECK(launch_agglo(d_packed, ctx->num, method, d_pairs, d_score, d_scratch, (hipStream_t)stream), return 1);
		return 0;
	});
}

extern "C" double sa_hip_last_agglomerate_seconds(void)
{
	return sa_guard("sa_hip_last_agglomerate_seconds", 0.0, [&] { return g_last_agglo_seconds.load(); });
}

extern "C" int64_t sa_hip_last_agglomerate_rescans(void)
{
	return sa_guard("sa_hip_last_agglomerate_rescans", (int64_t)0, [&] { return g_last_agglo_rescans.load(); });
}

/* ---- host only: the labels of such a tree ------------------------------------------------------------------------------------ */
extern "C" int32_t sa_agglo_labels(const int32_t *pairs, const int32_t *score, int32_t num, int32_t min_score, int32_t *labels)
{
	return sa_guard("sa_agglo_labels", (int32_t)-1, [&]() -> int32_t {
		if (!labels || (num > 1 && (!pairs || !score))) {
			sa_set_error("sa_agglo_labels: null argument");
			return -1;
		}
		if (num < 1) {
			sa_set_error("sa_agglo_labels: %d sequences", num);
			return -1;
		}
		const int32_t clusters = sa_ag_labels(pairs, score, num, min_score, labels);
		if (clusters < 0)
			sa_set_error("sa_agglo_labels: %s", ag_message(clusters));
		return clusters < 0 ? -1 : clusters;
	});
}
