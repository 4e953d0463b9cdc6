/* remainder_tiles_test.cpp -- the half and quarter tiles of the launch planner (sequencealigner_amd/csrc/sa_plan.cpp,
 * SaPlanInputs::remainder; the piece rule sa_pk_piece_window of sa_shapes.h) on the CPU, under ASan / UBSan
 * (tests/test_remainder_tiles_host.py builds and runs it).  Two stores -- 2300 sequences of 17..190 residues (8-lane groups,
 * NW: K = 3..24, the eight-wave classes among them) and 700 of 200..260 (16-lane groups, Gotoh) -- and for each the sweep
 * ranges {whole triangle, start and end inside columns, start and end on column boundaries, a bounded search range} x world
 * {0, 1, 2, 3, 8} x env_chunk {0, 8, 16, 32} x {device, host} output x {-, no_sort, no_tokens}.  Every plan is checked from
 * its lists alone, the way the kernel derives a tile (sa_systolic_pk.inc: pk_tile's prologue with the row window):
 *   - every (row, column) of the range lies in exactly one tile; a share plan's segments place every pair exactly once;
 *   - every half or quarter tile lies inside its pair's row range, is aligned to its size, has all its rows, picks its own
 *     arranged block (and its segments carry flags bit 0);
 *   - the residual partial tile is smaller than the smallest shape the plan offers (a quarter tile where those exist);
 *   - sa_build_tokens / sa_build_row_streams accept the arranged copy of every new {ng, ch} (the window check);
 *   - the plan's lean count exceeds that of the plan without remainder tiles by the number of half and quarter tiles;
 *   - without remainder tiles (the switch) the tile lists are the rule "full tiles, one partial per pair" recomputed naively
 *     and no variant class exists.
 * Prints "ok <plans>" and exits 0, or says what differs and exits 1. */
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_plan.h"

extern "C" const char *sa_last_error(void);

static int g_fail = 0;
#define CHECK(cond, ...)                                                             \
	do {                                                                         \
		if (!(cond)) {                                                       \
			fprintf(stderr, "CHECK FAILED %s:%d: ", __FILE__, __LINE__); \
			fprintf(stderr, __VA_ARGS__);                                \
			fprintf(stderr, "\n");                                       \
			if (++g_fail > 20)                                           \
				exit(1);                                             \
		}                                                                    \
	} while (0)

struct Tile {
	int32_t j[2], ia[2], ib[2], ra0, rb0, i_begin, i_count, rows;
	bool dup, full;
};

/* tile t of a packed class from the class's lists, as pk_tile's prologue derives it */
static Tile tile_of(const SaPlanInputs &in, const SaHostPlan &pl, const SaHostClass &cl, int32_t t)
{
	Tile g{};
	const int64_t start = pl.start, end = pl.start + pl.count;
	const SaPkCls pc = sa_pk_decode(cl.cls);
	g.rows = sa_pk_wpb(in.method, pc.g, pc.k) * (64 / pc.g) * cl.chunk;
	const int32_t npairs = (cl.ncols + 1) / 2, nfull = cl.tprefix[(size_t)npairs];
	g.full = t < nfull;
	int32_t lo;
	if (t < nfull)
		lo = (int32_t)(std::upper_bound(cl.tprefix.begin(), cl.tprefix.begin() + npairs + 1, t) - cl.tprefix.begin()) - 1;
	else
		lo = cl.tprefix[(size_t)(npairs + 1 + (t - nfull))];
	const size_t c0 = (size_t)2 * (size_t)lo, c1 = c0 + 1 < cl.jlist.size() ? c0 + 1 : c0;
	g.dup = c0 == c1;
	g.j[0] = cl.jlist[c0], g.j[1] = cl.jlist[c1];
	for (int h = 0; h < 2; h++) {
		const int64_t j = g.j[h], tri = sa_tri(j);
		const int64_t a = start > tri ? start - tri : 0;
		const int64_t jb = in.row_end && in.row_end < j ? in.row_end : j;
		const int64_t b = end - tri < jb ? end - tri : jb;
		g.ia[h] = (int32_t)a;
		g.ib[h] = (int32_t)(b > a ? b : a);
	}
	int32_t ra = std::min(g.ia[0], g.ia[1]), rb = std::max(g.ib[0], g.ib[1]);
	g.ra0 = ra, g.rb0 = rb;
	if (cl.piece) {
		int32_t wlo, whi;
		sa_pk_piece_window(ra, rb, g.rows << (cl.piece & 3), cl.piece, wlo, whi);
		for (int h = 0; h < 2; h++) {
			g.ia[h] = sa_pk_clamp(g.ia[h], wlo, whi);
			g.ib[h] = sa_pk_clamp(g.ib[h], wlo, whi);
		}
		ra = wlo, rb = whi;
	}
	const int32_t chunk = t < nfull ? t - cl.tprefix[(size_t)lo] : cl.tprefix[(size_t)lo + 1] - cl.tprefix[(size_t)lo];
	g.i_begin = ra + chunk * g.rows;
	g.i_count = std::min(g.rows, rb - g.i_begin);
	return g;
}

struct Store {
	std::vector<int32_t> lens;
	std::vector<sa_meta> meta;
	std::map<std::tuple<int, int, int32_t, uint32_t>, bool> streams_ok; /* (key, stride) -> the builders accepted it */
	std::map<std::tuple<int, int, int32_t>, std::vector<int32_t>> rowmaps;
};

static const std::vector<int32_t> &rowmap_of(Store &st, const SaArrKey &key)
{
	auto k = std::make_tuple(key.ng, key.ch, key.block);
	auto it = st.rowmaps.find(k);
	if (it == st.rowmaps.end()) {
		std::vector<int32_t> rm;
		sa_arrange_rows(st.meta.data(), (int32_t)st.lens.size(), key, rm);
		it = st.rowmaps.emplace(k, std::move(rm)).first;
	}
	return it->second;
}

/* the arranged copy of the store for `key`, its token streams and -- where the class reads them -- its row streams */
static bool streams_build(Store &st, const SaArrKey &key, uint32_t stride)
{
	auto k = std::make_tuple(key.ng, key.ch, key.block, stride);
	auto it = st.streams_ok.find(k);
	if (it != st.streams_ok.end())
		return it->second;
	const std::vector<int32_t> &rm = rowmap_of(st, key);
	std::vector<uint8_t> codes;
	std::vector<int32_t> off(1, 0);
	unsigned seed = 5u;
	for (int32_t row : rm) {
		for (int32_t q = 0; q < st.lens[(size_t)row]; q++) {
			seed = seed * 1664525u + 1013904223u;
			codes.push_back((uint8_t)((seed >> 16) % 24u));
		}
		codes.push_back((uint8_t)SA_CODE_SEP);
		off.push_back((int32_t)codes.size());
	}
	SaTokenStreams ts;
	std::vector<uint32_t> rows;
	bool ok = sa_build_tokens(codes.data(), off.data(), (int32_t)st.lens.size(), key, ts) && ts.streams > 0;
	if (ok && stride)
		ok = sa_build_row_streams(ts, key.ng, stride, rows) && !rows.empty();
	st.streams_ok[k] = ok;
	return ok;
}

struct Counts {
	int64_t lean = 0, pieces = 0, tiles = 0;
};

static Counts check_plan(Store &st, const SaPlanInputs &in, const SaHostPlan &pl, const char *what)
{
	Counts n;
	const int64_t start = pl.start, end = pl.start + pl.count;
	const int32_t j0 = sa_column_of(start), j1 = sa_column_of(end - 1);
	std::vector<std::vector<uint8_t>> seen((size_t)(j1 - j0 + 1));
	for (int32_t j = j0; j <= j1; j++)
		seen[(size_t)(j - j0)].assign((size_t)j, 0);
	CHECK(pl.generic.empty(), "%s: the stores of this test are all packed classes", what);
	std::map<std::pair<int64_t, int32_t>, const SaHostSeg *> seg_at; /* (dst, pos0) -> segment */
	for (const auto &sg : pl.segs)
		seg_at[{ sg.dst, sg.pos0 }] = &sg;
	for (const auto &b : pl.bundles) {
		CHECK(b.cls.size() <= ((size_t)1 << (32 - SA_PK_UTILE_BITS)), "%s: a bundle of %zu classes overflows the tile code", what, b.cls.size());
		for (size_t x = 0; x < b.cls.size(); x++) {
			const SaHostClass &cl = pl.classes[(size_t)b.cls[x]];
			const SaPkCls pc = sa_pk_decode(cl.cls);
			const int variant = cl.piece & 3, avail = cl.piece >> 2;
			CHECK(pc.variant == variant && b.args[x].piece == cl.piece && b.args[x].chunk == cl.chunk, "%s: class %d: piece %d, variant %d", what, cl.cls,
			      cl.piece, pc.variant);
			CHECK(in.remainder || cl.piece == 0, "%s: class %d has a row window without remainder tiles", what, cl.cls);
			CHECK(cl.ntiles > 0, "%s: class %d has no tile", what, cl.cls);
			if (variant)
				CHECK((avail & (1 << (variant - 1))) && cl.chunk >= 4, "%s: class %d: variant %d of chunk %d not on offer (%d)", what, cl.cls, variant,
				      cl.chunk, avail);
			const auto &lv = b.args[x].lv;
			const int32_t lvrows[SA_PK_SORT_LEVELS] = { lv[0].block, lv[1].block, lv[2].block, lv[3].block };
			int64_t pairs = 0;
			for (int32_t t = 0; t < cl.ntiles; t++) {
				const Tile g = tile_of(in, pl, cl, t);
				n.tiles++;
				CHECK(g.i_count > 0 && g.i_begin >= 0 && g.i_begin + g.i_count <= in.num, "%s: class %d tile %d: rows [%d,+%d)", what, cl.cls, t, g.i_begin,
				      g.i_count);
				if (g.i_count <= 0)
					continue;
				if (!g.full)
					CHECK(g.i_count == cl.part_rows[(size_t)(t - (cl.ntiles - cl.npart))], "%s: class %d tile %d: %d rows, part_rows says %d", what,
					      cl.cls, t, g.i_count, cl.part_rows[(size_t)(t - (cl.ntiles - cl.npart))]);
				const int32_t ra = std::min(g.ia[0], g.ia[1]), rb = std::max(g.ib[0], g.ib[1]);
				const int l = sa_pk_pick_level(lvrows, ra, rb, g.i_begin, g.rows);
				if (l >= 0 && !in.no_tokens)
					n.lean++;
				CHECK(l < 0 || g.full, "%s: class %d tile %d: a partial tile picked an arranged level", what, cl.cls, t);
				if (variant && g.full) { /* a half or quarter tile */
					n.pieces++;
					CHECK(g.i_count == g.rows && g.i_begin % g.rows == 0, "%s: class %d tile %d: piece [%d,+%d) of %d-row shape", what, cl.cls, t,
					      g.i_begin, g.i_count, g.rows);
					CHECK(g.i_begin >= g.ra0 && g.i_begin + g.i_count <= g.rb0, "%s: class %d tile %d: piece [%d,+%d) outside the pair's rows [%d,%d)",
					      what, cl.cls, t, g.i_begin, g.i_count, g.ra0, g.rb0);
					CHECK(l >= 0 && lv[l].block == g.rows && lv[l].ch == cl.chunk, "%s: class %d tile %d: piece is not its own arranged block (level %d)",
					      what, cl.cls, t, l);
					if (l >= 0) {
						const uint32_t stride = sa_pk_reg_tokens(in.method, pc.g, pc.k) && !in.no_tokens ? sa_pk_row_stride(pc.k) : 0u;
						CHECK(streams_build(st, lv[l], stride), "%s: class %d: streams of {%d, %d, %d} stride %u refused: %s", what, cl.cls, lv[l].ng,
						      lv[l].ch, lv[l].block, stride, sa_last_error());
					}
					if (pl.world >= 1)
						for (int h = 0; h < (g.dup ? 1 : 2); h++) {
							auto it = seg_at.find({ sa_tri(g.j[h]) - start, g.i_begin });
							CHECK(it != seg_at.end() && it->second->count == g.i_count && (it->second->flags & 1) && it->second->map_kind == 2 &&
								      it->second->ia == g.ia[h] && it->second->ib == g.ib[h],
							      "%s: class %d tile %d: no own-block segment for column %d", what, cl.cls, t, g.j[h]);
						}
				}
				if (cl.piece && !g.full && g.ra0 % (g.rows << variant) == 0) { /* the residual (a pair off the tile grid is not cut) */
					const int32_t smallest = (g.rows << variant) >> ((avail & 2) ? 2 : 1);
					CHECK(g.i_count < smallest, "%s: class %d tile %d: residual of %d rows, the smallest shape on offer has %d", what, cl.cls, t,
					      g.i_count, smallest);
				}
				for (int h = 0; h < (g.dup ? 1 : 2); h++)
					for (int32_t r = std::max(g.ia[h], g.i_begin); r < std::min(g.ib[h], g.i_begin + g.i_count); r++) {
						CHECK(g.j[h] >= j0 && g.j[h] <= j1 && r < g.j[h], "%s: class %d tile %d: (%d, %d) outside the range", what, cl.cls, t, r, g.j[h]);
						seen[(size_t)(g.j[h] - j0)][(size_t)r]++;
						pairs++;
					}
			}
			CHECK(pairs == cl.pairs, "%s: class %d: tiles cover %" PRId64 " pairs, the class claims %" PRId64, what, cl.cls, pairs, cl.pairs);
		}
	}
	int64_t bad = 0;
	for (int32_t j = j0; j <= j1; j++) {
		const int64_t tri = sa_tri(j);
		const int64_t a = std::max<int64_t>(0, start - tri);
		const int64_t b = std::min<int64_t>(in.row_end && in.row_end < j ? in.row_end : j, end - tri);
		for (int32_t r = 0; r < j; r++)
			bad += seen[(size_t)(j - j0)][(size_t)r] != (r >= a && r < b ? 1 : 0);
	}
	CHECK(bad == 0, "%s: %" PRId64 " (row, column) not covered exactly once", what, bad);
	int64_t lean_plan = 0;
	for (const auto &b : pl.bundles)
		for (int64_t v : b.tok_lean)
			lean_plan += v;
	CHECK(lean_plan == n.lean, "%s: the plan counts %" PRId64 " lean tiles, the tiles say %" PRId64, what, lean_plan, n.lean);
	if (pl.world >= 1) { /* placement: every pair of the range exactly once */
		std::vector<uint8_t> placed((size_t)pl.count, 0);
		int64_t twice = 0, outside = 0;
		for (const auto &sg : pl.segs) {
			const std::vector<int32_t> *rm = sg.map_kind ? &rowmap_of(st, sg.key) : nullptr;
			for (int32_t q = sg.pos0; q < sg.pos0 + sg.count; q++) {
				if (q >= in.num)
					break;
				const int32_t r = rm ? (*rm)[(size_t)q] : q;
				if (r < sg.ia || r >= sg.ib)
					continue;
				const int64_t e = sg.dst + r;
				if (e < 0 || e >= pl.count)
					outside++;
				else if (placed[(size_t)e]++)
					twice++;
			}
		}
		int64_t missing = 0;
		for (uint8_t v : placed)
			missing += v == 0;
		CHECK(!twice && !outside && !missing, "%s: placement: %" PRId64 " pairs twice, %" PRId64 " outside, %" PRId64 " never", what, twice, outside, missing);
	}
	return n;
}

/* the plan without remainder tiles: full tiles of the class's chunk, one partial per pair, partials by decreasing size */
static void check_parent_rule(const SaPlanInputs &in, const SaHostPlan &pl, const char *what)
{
	for (const auto &cl : pl.classes) {
		const SaPkCls pc = sa_pk_decode(cl.cls);
		CHECK(pc.variant == SA_PK_MAIN && cl.piece == 0, "%s: class %d is a variant", what, cl.cls);
		CHECK(cl.chunk == (pc.small ? pl.chunk_pk_small : pl.chunk_pk), "%s: class %d: chunk %d", what, cl.cls, cl.chunk);
		const int32_t rows = sa_pk_wpb(in.method, pc.g, pc.k) * (64 / pc.g) * cl.chunk;
		std::vector<int32_t> tp(1, 0);
		std::vector<std::pair<int32_t, int32_t>> parts;
		for (size_t c = 0; c < cl.jlist.size(); c += 2) {
			int32_t ra = INT32_MAX, rb = 0;
			for (size_t h = c; h < std::min(c + 2, cl.jlist.size()); h++) {
				const int64_t j = cl.jlist[h], tri = sa_tri(j);
				const int64_t a = std::max<int64_t>(0, pl.start - tri);
				int64_t b = std::min<int64_t>(j, pl.start + pl.count - tri);
				if (in.row_end)
					b = std::min<int64_t>(b, in.row_end);
				ra = std::min(ra, (int32_t)a);
				rb = std::max(rb, (int32_t)b);
			}
			tp.push_back(tp.back() + (rb - ra) / rows);
			if ((rb - ra) % rows)
				parts.emplace_back((rb - ra) % rows, (int32_t)(c / 2));
		}
		std::stable_sort(parts.begin(), parts.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
		std::vector<int32_t> part_rows;
		for (const auto &p : parts) {
			tp.push_back(p.second);
			part_rows.push_back(p.first);
		}
		CHECK(tp == cl.tprefix && part_rows == cl.part_rows && cl.npart == (int32_t)parts.size() &&
			      cl.ntiles == tp[(cl.jlist.size() + 1) / 2] + cl.npart,
		      "%s: class %d: the tile list is not the parent's rule", what, cl.cls);
	}
}

int main()
{
	int plans = 0;
	int64_t pieces_all = 0;
	struct Case {
		int32_t num, lo, hi;
		int method;
		int32_t n_db; /* of the bounded range */
	} const cases[] = { { 2300, 17, 190, SA_METHOD_NW, 1500 }, { 700, 200, 260, SA_METHOD_GA, 450 } };
	for (const Case &cs : cases) {
		Store st;
		unsigned seed = 1234u + (unsigned)cs.num;
		for (int32_t k = 0; k < cs.num; k++) {
			seed = seed * 1664525u + 1013904223u;
			st.lens.push_back(cs.lo + (int32_t)((seed >> 16) % (unsigned)(cs.hi - cs.lo + 1)));
		}
		int64_t off = 0;
		for (int32_t len : st.lens) {
			st.meta.push_back(sa_meta{ (int32_t)off, len });
			off += len + 1;
		}
		SaPlanInputs base;
		base.num = cs.num;
		base.meta = st.meta.data();
		base.min_len = cs.lo;
		base.method = cs.method;
		base.gap_ext = -1;
		base.sys_ok = true;
		base.pk_kmax = SA_PK_KMAX;
		base.pk16_kmax = SA_PK16_KMAX;
		base.pk16_f16_kmax = SA_PK16_F16_KMAX;
		base.pk_q = -9;
		base.pk_floor = 100;
		base.pk_gain = 1;
		base.pk_slack = 12;
		const int64_t all = sa_tri(cs.num);
		struct Range {
			int64_t start, end;
			int32_t row_end;
		} const ranges[] = {
			{ 0, all, 0 },
			{ sa_tri(cs.num / 3) + 77, sa_tri(cs.num - 40) + 301, 0 },
			{ sa_tri(cs.num / 4), sa_tri(cs.num - 3), 0 },
			{ sa_tri(cs.n_db + 5), sa_tri(cs.num - 2), cs.n_db },
		};
		for (const Range &rg : ranges)
			for (int world : { 0, 1, 2, 3, 8 })
				for (int chunk : { 0, 8, 16, 32 })
					for (int host = 0; host < 2; host++)
						for (int flags = 0; flags < 3; flags++) {
							if (rg.row_end && world >= 1)
								continue; /* (a bounded plan goes with no share plan) */
							if (flags && (host || (world != 0 && world != 3)))
								continue; /* (the two switches: device output, the plain plan and one share plan) */
							SaPlanInputs in = base;
							in.env_chunk = chunk;
							in.row_end = rg.row_end;
							in.no_sort = flags == 1;
							in.no_tokens = flags == 2;
							char what[160];
							snprintf(what, sizeof(what), "num %d [%" PRId64 ",%" PRId64 ") row_end %d world %d chunk %d host %d flags %d", cs.num, rg.start,
								 rg.end, rg.row_end, world, chunk, host, flags);
							SaHostPlan off_plan, on_plan;
							if (!sa_plan_host(in, rg.start, rg.end - rg.start, world, host != 0, off_plan)) {
								CHECK(false, "%s: refused: %s", what, sa_last_error());
								continue;
							}
							check_parent_rule(in, off_plan, what);
							const Counts c0 = check_plan(st, in, off_plan, what);
							in.remainder = true;
							if (!sa_plan_host(in, rg.start, rg.end - rg.start, world, host != 0, on_plan)) {
								CHECK(false, "%s: with remainder tiles: refused: %s", what, sa_last_error());
								continue;
							}
							const Counts c1 = check_plan(st, in, on_plan, what);
							CHECK(c0.pieces == 0, "%s: %" PRId64 " pieces without remainder tiles", what, c0.pieces);
							CHECK(in.no_tokens ? c1.lean == 0 : c1.lean == c0.lean + c1.pieces, "%s: lean tiles %" PRId64 " -> %" PRId64 " with %" PRId64 " pieces",
							      what, c0.lean, c1.lean, c1.pieces);
							/* (a pair whose last rows are exactly its pieces has no residual any more) */
							CHECK(c1.tiles <= c0.tiles + c1.pieces && c1.tiles >= c0.tiles, "%s: %" PRId64 " -> %" PRId64 " tiles with %" PRId64 " pieces", what, c0.tiles,
							      c1.tiles, c1.pieces);
							if (in.no_sort)
								CHECK(c1.pieces == 0, "%s: pieces without arranged copies", what);
							else if (chunk == 16 || chunk == 32)
								CHECK(c1.pieces > 0, "%s: no half or quarter tile at chunk %d", what, chunk);
							pieces_all += c1.pieces;
							plans += 2;
						}
	}
	if (g_fail) {
		fprintf(stderr, "%d check(s) failed\n", g_fail);
		return 1;
	}
	printf("ok %d plans, %" PRId64 " half and quarter tiles\n", plans, pieces_all);
	return 0;
}
