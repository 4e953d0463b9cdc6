/* search_plan_test.cpp -- the row bound of the launch planner (sequencealigner_amd/csrc/sa_plan.cpp: SaPlanInputs::row_end)
 * under ASan / UBSan, as a search context uses it (csrc/sa_search.hip).  Built with sa_plan.cpp, sa_limits.cpp and the matrix
 * tables, and run by tests/test_search_host.py.
 *
 *   search_plan_test <lens.i32> <N> <method> <matrix> <gap_pen> <gap_open> <gap_ext> <CUs> <force_generic> <no_pk>
 *
 * lens.i32 holds the lengths of the concatenated store: N database sequences, then M queries.  For the query ranges
 * (q0, nq) = (0, M), (17, 1), (M - 3, 3) -- those that exist -- the plan of [tri(N + q0), tri(N + q0 + nq)) with row_end = N is
 * built and checked from its lists alone, the way the kernels derive a tile (the prologues of sa_systolic_pk.inc and
 * sa_systolic_kernel.inc, with the clamp):
 *   - every (d, q) with d < N is in exactly one tile or generic run, no tile or run has a row >= N,
 *   - the plan's pair count -- classes, bundles, generic runs -- is nq * N,
 *   - a generic run is one column's rows [tri(j), +N).
 * Then: a bounded plan with world = 1 is refused; row_end = 0 gives a plan equal, field for field, to one built from inputs
 * whose field was never touched (for the whole triangle and for the unbounded tail range). */
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...) \
	do { \
		if (!(cond)) { \
			fprintf(stderr, "CHECK FAILED %s:%d: ", __FILE__, __LINE__); \
			fprintf(stderr, __VA_ARGS__); \
			fprintf(stderr, "\n"); \
			if (++g_fail > 20) \
				exit(1); \
		} \
	} while (0)

static void check_bounded(const SaPlanInputs &in, int32_t n_db, int32_t q0, int32_t nq)
{
	const int64_t start = sa_tri((int64_t)n_db + q0), end = sa_tri((int64_t)n_db + q0 + nq);
	SaHostPlan pl;
	if (!sa_plan_host(in, start, end - start, 0, false, pl)) {
		CHECK(false, "queries [%d,+%d): refused: %s", q0, nq, sa_last_error());
		return;
	}
	std::vector<int32_t> seen((size_t)nq * (size_t)n_db, 0);
	auto rows_of = [&](int32_t j, int32_t &ia, int32_t &ib) { /* the kernels' prologue */
		const int64_t tri = sa_tri(j);
		const int64_t a = start > tri ? start - tri : 0;
		const int64_t jb = in.row_end && in.row_end < j ? in.row_end : j;
		const int64_t b = end - tri < jb ? end - tri : jb;
		ia = (int32_t)a;
		ib = (int32_t)(b > a ? b : a);
	};
	auto mark = [&](int32_t j, int64_t lo, int64_t hi, const char *what) {
		CHECK(j >= n_db + q0 && j < n_db + q0 + nq, "%s: column %d outside the queries", what, j);
		CHECK(lo >= 0 && hi <= n_db, "%s: rows [%" PRId64 ", %" PRId64 ") of column %d pass the database (%d)", what, lo, hi, j, n_db);
		if (j < n_db + q0 || j >= n_db + q0 + nq)
			return;
		for (int64_t d = std::max<int64_t>(lo, 0); d < std::min<int64_t>(hi, n_db); d++)
			seen[(size_t)(j - n_db - q0) * (size_t)n_db + (size_t)d]++;
	};
	int64_t pairs = 0, pk_pairs = 0, bundle_pairs = 0;
	for (const auto &cl : pl.classes) {
		pairs += cl.pairs;
		int64_t mine = 0;
		for (int32_t t = 0; t < cl.ntiles; t++) {
			int32_t j[2], ia[2], ib[2], i_begin, i_count;
			bool dup = true;
			if (cl.cls >= SA_PK_CLASS0) {
				const SaPkCls pc = sa_pk_decode(cl.cls);
				const int32_t rows = sa_pk_wpb(in.method, pc.g, pc.k) * (64 / pc.g) * cl.chunk;
				const int32_t npairs = (cl.ncols + 1) / 2, nfull = cl.tprefix[(size_t)npairs];
				int32_t lo;
				if (t < nfull)
					lo = (int32_t)(std::upper_bound(cl.tprefix.begin(), cl.tprefix.begin() + npairs + 1, t) - cl.tprefix.begin()) - 1;
				else
					lo = cl.tprefix[(size_t)(npairs + 1 + (t - nfull))];
				const size_t c0 = (size_t)2 * (size_t)lo, c1 = c0 + 1 < cl.jlist.size() ? c0 + 1 : c0;
				dup = c0 == c1;
				j[0] = cl.jlist[c0], j[1] = cl.jlist[c1];
				rows_of(j[0], ia[0], ib[0]);
				rows_of(j[1], ia[1], ib[1]);
				const int32_t ra = std::min(ia[0], ia[1]), rb = std::max(ib[0], ib[1]);
				const int32_t chunk = t < nfull ? t - cl.tprefix[(size_t)lo] : cl.tprefix[(size_t)lo + 1] - cl.tprefix[(size_t)lo];
				i_begin = ra + chunk * rows;
				i_count = std::min(rows, rb - i_begin);
			} else {
				const int G = cl.cls == SA_SYS_CLASS_LONG ? 64 : SA_SYS_CLASSES[cl.cls].G;
				const int rows = cl.cls == SA_SYS_CLASS_LONG ? SA_SYS_WPB(64, true) * std::min(pl.chunk, 16) : SA_SYS_WPB(G, false) * (64 / G) * pl.chunk;
				const int32_t k = (int32_t)(std::upper_bound(cl.tprefix.begin(), cl.tprefix.end(), t) - cl.tprefix.begin()) - 1;
				j[0] = j[1] = cl.jlist[(size_t)k];
				rows_of(j[0], ia[0], ib[0]);
				ia[1] = ia[0], ib[1] = ib[0];
				i_begin = ia[0] + (t - cl.tprefix[(size_t)k]) * rows;
				i_count = std::min(rows, ib[0] - i_begin);
			}
			CHECK(i_count > 0, "class %d tile %d: empty", cl.cls, t);
			CHECK(i_begin >= 0 && i_begin + i_count <= n_db, "class %d tile %d: rows [%d,+%d) pass the database (%d)", cl.cls, t, i_begin, i_count, n_db);
			for (int h = 0; h < (dup ? 1 : 2); h++) {
				const int64_t lo = std::max(ia[h], i_begin), hi = std::min(ib[h], i_begin + i_count);
				if (hi > lo) {
					mark(j[h], lo, hi, "tile");
					mine += hi - lo;
				}
			}
		}
		CHECK(mine == cl.pairs, "class %d: tiles cover %" PRId64 " pairs, class claims %" PRId64, cl.cls, mine, cl.pairs);
		if (cl.cls >= SA_PK_CLASS0)
			pk_pairs += cl.pairs;
	}
	for (const auto &b : pl.bundles) {
		CHECK(b.pairs.size() == 1 && b.nlocal.size() == 1, "bundle of a plan without shares: %zu ranks", b.pairs.size());
		bundle_pairs += b.pairs[0];
		int64_t tiles = 0;
		for (int ci : b.cls)
			tiles += pl.classes[(size_t)ci].ntiles;
		CHECK(b.nlocal[0] == tiles && b.tok_lean[0] + b.tok_legacy[0] == tiles, "bundle: %d tiles listed, %" PRId64 " in its classes", b.nlocal[0], tiles);
	}
	CHECK(bundle_pairs == pk_pairs, "bundles claim %" PRId64 " pairs, their classes %" PRId64, bundle_pairs, pk_pairs);
	for (const auto &run : pl.generic) {
		const int32_t j = sa_column_of(run.first);
		CHECK(run.first == sa_tri(j) && run.second == n_db, "generic run [%" PRId64 ",+%" PRId64 ") is not the database rows of column %d", run.first,
		      run.second, j);
		mark(j, run.first - sa_tri(j), run.first - sa_tri(j) + run.second, "generic run");
		pairs += run.second;
	}
	CHECK(pairs == (int64_t)nq * n_db, "queries [%d,+%d): the plan counts %" PRId64 " pairs, nq * N = %" PRId64, q0, nq, pairs, (int64_t)nq * n_db);
	int64_t bad = 0;
	for (int32_t v : seen)
		bad += v != 1;
	CHECK(bad == 0, "queries [%d,+%d): %" PRId64 " of %zu (d, q) not covered exactly once", q0, nq, bad, seen.size());
	printf("bounded plan ok: queries [%d,+%d) x %d: %zu classes, %zu bundles, %zu generic runs, %" PRId64 " pairs\n", q0, nq, n_db, pl.classes.size(),
	       pl.bundles.size(), pl.generic.size(), pairs);
}

/* ---- field-for-field equality of two plans ---- */
static bool same_key(const SaArrKey &a, const SaArrKey &b) { return a == b; }
static bool same_class(const SaHostClass &a, const SaHostClass &b)
{
	return a.cls == b.cls && a.ncols == b.ncols && a.ntiles == b.ntiles && a.npart == b.npart && a.chunk == b.chunk && a.pairs == b.pairs &&
	       a.cells == b.cells && a.jlist == b.jlist && a.tprefix == b.tprefix && a.part_rows == b.part_rows && a.tlist == b.tlist && a.doff == b.doff &&
	       a.owner == b.owner && a.rank_first == b.rank_first && a.rank_pairs == b.rank_pairs && a.rank_cells == b.rank_cells;
}
static bool same_bundle(const SaHostBundle &a, const SaHostBundle &b)
{
	if (!(a.g == b.g && a.klo == b.klo && a.f16 == b.f16 && a.kmax == b.kmax && a.cls == b.cls && a.ulist == b.ulist && a.ufirst == b.ufirst &&
	      a.nlocal == b.nlocal && a.pairs == b.pairs && a.cells == b.cells && a.tok_lean == b.tok_lean && a.tok_legacy == b.tok_legacy &&
	      a.args.size() == b.args.size()))
		return false;
	for (size_t x = 0; x < a.args.size(); x++) {
		const SaHostPkArgs &p = a.args[x], &q = b.args[x];
		if (!(p.cls_index == q.cls_index && p.ncols == q.ncols && p.npart == q.npart && p.k == q.k && p.delta == q.delta && p.pk_base == q.pk_base &&
		      p.chunk == q.chunk))
			return false;
		for (int l = 0; l < SA_PK_SORT_LEVELS; l++)
			if (!same_key(p.lv[l], q.lv[l]))
				return false;
	}
	return true;
}
static bool same_plan(const SaHostPlan &a, const SaHostPlan &b)
{
	if (!(a.start == b.start && a.count == b.count && a.chunk == b.chunk && a.chunk_pk == b.chunk_pk && a.chunk_pk_small == b.chunk_pk_small &&
	      a.j_small == b.j_small && a.generic == b.generic && a.world == b.world && a.share_host == b.share_host && a.share_elems == b.share_elems &&
	      a.classes.size() == b.classes.size() && a.bundles.size() == b.bundles.size() && a.segs.size() == b.segs.size() &&
	      a.generic_share.size() == b.generic_share.size()))
		return false;
	for (size_t k = 0; k < a.classes.size(); k++)
		if (!same_class(a.classes[k], b.classes[k]))
			return false;
	for (size_t k = 0; k < a.bundles.size(); k++)
		if (!same_bundle(a.bundles[k], b.bundles[k]))
			return false;
	for (size_t k = 0; k < a.segs.size(); k++) {
		const SaHostSeg &p = a.segs[k], &q = b.segs[k];
		if (!(p.src == q.src && p.dst == q.dst && p.count == q.count && p.pos0 == q.pos0 && p.ia == q.ia && p.ib == q.ib && p.flags == q.flags &&
		      p.map_kind == q.map_kind && same_key(p.key, q.key)))
			return false;
	}
	for (size_t r = 0; r < a.generic_share.size(); r++) {
		if (a.generic_share[r].size() != b.generic_share[r].size())
			return false;
		for (size_t k = 0; k < a.generic_share[r].size(); k++)
			if (!(a.generic_share[r][k].start == b.generic_share[r][k].start && a.generic_share[r][k].count == b.generic_share[r][k].count &&
			      a.generic_share[r][k].doff == b.generic_share[r][k].doff))
				return false;
	}
	return true;
}

int main(int argc, char **argv)
{
	if (argc != 11) {
		fprintf(stderr, "usage: search_plan_test lens.i32 N method matrix gap_pen gap_open gap_ext CUs force_generic no_pk\n");
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	std::vector<int32_t> lens((size_t)bytes / 4);
	if (fread(lens.data(), 4, lens.size(), f) != lens.size())
		return 2;
	fclose(f);
	const int32_t num = (int32_t)lens.size(), n_db = atoi(argv[2]), m = num - n_db;
	if (n_db < 1 || m < 1) {
		fprintf(stderr, "N = %d of %d sequences\n", n_db, num);
		return 2;
	}
	std::vector<sa_meta> meta((size_t)num);
	int32_t max_len = 0, min_len = INT32_MAX;
	int64_t off = 0;
	for (int32_t k = 0; k < num; k++) {
		meta[(size_t)k] = sa_meta{ (int32_t)off, lens[(size_t)k] };
		off += lens[(size_t)k] + 1;
		max_len = std::max(max_len, lens[(size_t)k]);
		min_len = std::min(min_len, lens[(size_t)k]);
	}
	sa_scoring sc{};
	sc.method = sa_method_parse(argv[3]);
	if (sc.method < 0 || sa_matrix_load(argv[4], sc.lut, sc.sub)) {
		fprintf(stderr, "%s\n", sa_last_error());
		return 2;
	}
	sc.gap_pen = -atoi(argv[5]);
	sc.gap_opn = -atoi(argv[6]);
	sc.gap_ext = -atoi(argv[7]);
	const SaKernelLimits L = sa_kernel_limits(sc, max_len, min_len, atoi(argv[9]) != 0, atoi(argv[10]) != 0, false);
	SaPlanInputs in; /* row_end is NOT touched here: `in` is the inputs of a build that does not know the field */
	in.num = num;
	in.meta = meta.data();
	in.min_len = min_len;
	in.method = sc.method;
	in.gap_ext = sc.gap_ext;
	in.sys_ok = L.sys_ok;
	in.pk_kmax = L.pk_kmax;
	in.pk16_kmax = L.pk16_kmax;
	in.pk16_f16_kmax = L.pk16_f16_kmax;
	in.pk_chunk_cap = L.pk_chunk_cap;
	in.pk_q = L.pk_q;
	in.pk_floor = L.pk_floor;
	in.pk_gain = L.pk_gain;
	in.pk_slack = L.pk_slack;
	in.persistent_wgs = atoi(argv[8]) * 32;
	printf("store: %d + %d sequences, lengths %d..%d; limits: sys_ok %d pk_kmax %d pk16_kmax %d\n", n_db, m, min_len, max_len, (int)L.sys_ok, L.pk_kmax,
	       L.pk16_kmax);

	SaPlanInputs bounded = in;
	bounded.row_end = n_db;
	const int32_t ranges[3][2] = { { 0, m }, { 17, 1 }, { m - 3, 3 } };
	for (const auto &r : ranges)
		if (r[0] >= 0 && r[1] >= 1 && r[0] + r[1] <= m)
			check_bounded(bounded, n_db, r[0], r[1]);

	{ /* a bounded plan goes with no share plan */
		SaHostPlan pl;
		const int64_t start = sa_tri(n_db), count = sa_tri(num) - start;
		const bool ok = sa_plan_host(bounded, start, count, 1, false, pl);
		CHECK(!ok, "a bounded plan with world = 1 was accepted");
		if (!ok)
			printf("world = 1 refused: %s\n", sa_last_error());
		SaPlanInputs neg = in;
		neg.row_end = -1;
		CHECK(!sa_plan_host(neg, start, count, 0, false, pl), "row_end = -1 was accepted");
	}
	{ /* row_end = 0: the plans of today */
		SaPlanInputs zero = in;
		zero.row_end = 0;
		const int64_t all = sa_tri(num), tail = sa_tri(n_db);
		const int64_t cases[2][2] = { { 0, all }, { tail, all - tail } };
		for (const auto &c : cases)
			for (int world : { 0, 1, 3 }) {
				if (c[1] <= 0)
					continue;
				SaHostPlan a, b;
				const bool oa = sa_plan_host(in, c[0], c[1], world, false, a), ob = sa_plan_host(zero, c[0], c[1], world, false, b);
				CHECK(oa && ob, "unbounded plan [%" PRId64 ",+%" PRId64 ") world %d refused: %s", c[0], c[1], world, sa_last_error());
				CHECK(same_plan(a, b), "row_end = 0 changes the plan of [%" PRId64 ",+%" PRId64 ") world %d", c[0], c[1], world);
				if (world == 0 && c[0] == tail && num > n_db + 1) { /* (and the bound does change it: the check above is not vacuous) */
					SaHostPlan d;
					CHECK(sa_plan_host(bounded, c[0], c[1], 0, false, d) && !same_plan(a, d), "the bounded tail plan equals the unbounded one");
				}
			}
		printf("row_end = 0 ok\n");
	}
	if (g_fail) {
		fprintf(stderr, "%d checks failed\n", g_fail);
		return 1;
	}
	printf("search plan ok\n");
	return 0;
}
