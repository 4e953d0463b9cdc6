/* token_streams_test.cpp -- sa_build_tokens (sequencealigner_amd/csrc/sa_plan.cpp) alone, on the CPU, under ASan / UBSan
 * (tests/test_token_streams_host.py builds and runs it): for the tile shapes {ng 8, ch 1 / 2 / 32} and {ng 4, ch 2} and
 * stores holding lengths 1, 15, 16, 17, streams of an exact multiple of 16 positions and very unequal streams in one wave,
 *   - every stream equals its sequences' codes in position order, SEP behind each, NOP to the padded end;
 *   - the padded length covers the kernel's lookahead (block nblk + 1 is read) and is what DESIGN 4.2 states;
 *   - every stream starts 4-byte aligned (in fact on a 16-position boundary, which the mask indexing needs);
 *   - mine / any equal the SEP positions recomputed naively.
 * Prints "ok <cases>" and exits 0, or says what differs and exits 1. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_plan.h"

extern "C" const char *sa_last_error(void);

static int failures = 0;
#define CHECK(cond, ...)                                  \
	do {                                              \
		if (!(cond)) {                            \
			if (failures++ < 20) {            \
				fprintf(stderr, __VA_ARGS__); \
				fputc('\n', stderr);      \
			}                                 \
		}                                         \
	} while (0)

struct Store {
	std::vector<uint8_t> codes;
	std::vector<int32_t> off;
};

/* the copy sa_arranged_store makes: sequences in position order, terminators included */
static Store lay_out(const std::vector<int32_t> &lens, const std::vector<int32_t> &rowmap, unsigned seed)
{
	Store s;
	s.off.push_back(0);
	for (int32_t row : rowmap) {
		for (int32_t k = 0; k < lens[(size_t)row]; k++) {
			seed = seed * 1664525u + 1013904223u;
			s.codes.push_back((uint8_t)((seed >> 16) % 24u));
		}
		s.codes.push_back((uint8_t)SA_CODE_SEP);
		s.off.push_back((int32_t)s.codes.size());
	}
	return s;
}

static void check(const char *name, const Store &st, int32_t num, const SaArrKey &key)
{
	SaTokenStreams ts;
	if (!sa_build_tokens(st.codes.data(), st.off.data(), num, key, ts)) {
		CHECK(false, "%s: builder failed: %s", name, sa_last_error());
		return;
	}
	const int ng = key.ng, ch = key.ch, g = 64 / ng;
	const int32_t streams = num / key.block * (key.block / ch);
	CHECK(ts.streams == streams && (int32_t)ts.tok_off.size() == streams + 1, "%s: %d streams, expected %d", name, ts.streams, streams);
	if (ts.streams != streams || (int32_t)ts.tok_off.size() != streams + 1)
		return;
	CHECK(ts.tok_off[0] == 0 && (size_t)ts.tok_off[(size_t)streams] == ts.tok.size(), "%s: offsets do not span tok", name);
	CHECK(ts.mine.size() * 16 == ts.tok.size() && ts.any.size() * 16 * (size_t)ng == ts.tok.size(), "%s: mask array sizes", name);
	for (int32_t w = 0; w < streams / ng; w++) {
		int32_t smax = 0;
		for (int s = w * ng; s < (w + 1) * ng; s++)
			smax = std::max(smax, st.off[(size_t)(s + 1) * ch] - st.off[(size_t)s * ch]);
		const int32_t steps = smax + g - 1, nblk = (steps + 15) / 16;
		const int32_t want = (steps + 15) / 16 * 16 + 32;
		std::vector<uint16_t> any((size_t)want / 16, 0);
		for (int s = w * ng; s < (w + 1) * ng; s++) {
			const int32_t at = ts.tok_off[(size_t)s], padded = ts.tok_off[(size_t)s + 1] - at;
			CHECK(padded == want, "%s: stream %d padded to %d, expected %d", name, s, padded, want);
			/* the last block of the main loop, nblk - 1, prefetches block nblk + 1: positions up to 16 (nblk + 2) - 1 */
			CHECK(padded >= 16 * (nblk + 2), "%s: stream %d: %d positions do not cover the lookahead of %d blocks", name, s, padded, nblk);
			CHECK(at % 16 == 0 && (2 * (int64_t)at) % 4 == 0, "%s: stream %d starts at position %d", name, s, at);
			if (padded != want)
				continue;
			/* naive stream: the sequences of positions [s ch, (s + 1) ch) one after the other */
			std::vector<uint16_t> naive;
			for (int32_t p = s * ch; p < (s + 1) * ch; p++) {
				for (int32_t k = st.off[(size_t)p]; k < st.off[(size_t)p + 1] - 1; k++)
					naive.push_back(st.codes[(size_t)k]);
				naive.push_back((uint16_t)SA_CODE_SEP);
			}
			CHECK((int32_t)naive.size() <= smax, "%s: stream %d longer than its wave's longest", name, s);
			naive.resize((size_t)padded, (uint16_t)SA_CODE_NOP);
			for (int32_t p = 0; p < padded; p++)
				CHECK(ts.tok[(size_t)at + (size_t)p] == naive[(size_t)p], "%s: stream %d position %d: token %d, expected %d", name, s, p,
				      ts.tok[(size_t)at + (size_t)p], naive[(size_t)p]);
			for (int32_t b = 0; b < padded / 16; b++) {
				uint16_t m = 0;
				for (int p = 0; p < 16; p++)
					if (naive[(size_t)(16 * b + p)] == SA_CODE_SEP)
						m |= (uint16_t)(1u << p);
				any[(size_t)b] |= m;
				CHECK(ts.mine[(size_t)(at / 16 + b)] == m, "%s: stream %d block %d: mine %04x, expected %04x", name, s, b,
				      ts.mine[(size_t)(at / 16 + b)], m);
			}
		}
		const int32_t any_at = ts.tok_off[(size_t)w * ng] / 16 / ng;
		for (int32_t b = 0; b < want / 16; b++)
			CHECK(ts.any[(size_t)(any_at + b)] == any[(size_t)b], "%s: wave slot %d block %d: any %04x, expected %04x", name, w, b,
			      ts.any[(size_t)(any_at + b)], any[(size_t)b]);
	}
}

int main()
{
	int cases = 0;
	const SaArrKey shapes[] = { { 8, 1, 0 }, { 8, 2, 0 }, { 8, 32, 0 }, { 4, 2, 0 } };
	for (const SaArrKey &shape : shapes) {
		SaArrKey key = shape;
		key.block = key.ng * key.ch * SA_PK_WPB * 2; /* two workgroup-tiles per arranged block */
		const int32_t num = 2 * key.block + key.block / 2 + 3; /* two full blocks and a tail that gets no streams */
		/* lengths: the edge cases again and again, a 190 beside 1s, and a spread */
		static const int32_t edge[] = { 1, 15, 16, 17, 1, 190, 1, 1, 31, 32, 33, 47, 48, 49, 2, 120 };
		std::vector<int32_t> lens((size_t)num);
		std::vector<sa_meta> meta((size_t)num);
		unsigned seed = 12345u + (unsigned)key.ch;
		for (int32_t k = 0; k < num; k++) {
			seed = seed * 1664525u + 1013904223u;
			lens[(size_t)k] = k % 3 == 0 ? edge[(size_t)(k / 3) % 16] : 1 + (int32_t)((seed >> 16) % 40u);
			meta[(size_t)k].len = lens[(size_t)k];
		}
		char name[96];
		/* (a) the arranged copy, as the context builds it */
		std::vector<int32_t> rowmap;
		sa_arrange_rows(meta.data(), num, key, rowmap);
		snprintf(name, sizeof(name), "arranged ng %d ch %d block %d", key.ng, key.ch, key.block);
		check(name, lay_out(lens, rowmap, 7u), num, key);
		cases++;
		/* (b) store order: the builder does not care, and neighbours of very unequal length share a wave */
		for (int32_t k = 0; k < num; k++)
			rowmap[(size_t)k] = k;
		snprintf(name, sizeof(name), "store order ng %d ch %d block %d", key.ng, key.ch, key.block);
		check(name, lay_out(lens, rowmap, 9u), num, key);
		cases++;
		/* (c) streams of exactly 16 k positions, one position less and one more: ch sequences of 16 k / ch - 1 (+-) residues */
		for (int d = -1; d <= 1; d++) {
			for (int32_t k = 0; k < num; k++) {
				const int32_t per = 16 * (1 + (k / key.ch) % 3) * (key.ch == 32 ? 4 : 1); /* positions of the stream: 16, 32, 48 (x4) */
				int32_t l = per / key.ch - 1;
				if (k % key.ch == 0)
					l += per % key.ch + d;
				lens[(size_t)k] = l < 1 ? 1 : l;
			}
			snprintf(name, sizeof(name), "16k%+d positions ng %d ch %d", d, key.ng, key.ch);
			check(name, lay_out(lens, rowmap, 11u), num, key);
			cases++;
		}
		/* (d) no full block: nothing is built */
		SaTokenStreams none;
		const bool ok = sa_build_tokens(nullptr, nullptr, key.block - 1, key, none);
		CHECK(ok && none.streams == 0 && none.tok.empty(), "no full block: %d streams", none.streams);
		cases++;
	}
	if (failures) {
		fprintf(stderr, "%d check(s) failed\n", failures);
		return 1;
	}
	printf("ok %d\n", cases);
	return 0;
}
