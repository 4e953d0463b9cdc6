/* row_streams_test.cpp -- sa_build_row_streams (sequencealigner_amd/csrc/sa_plan.cpp) alone, on the CPU, under ASan / UBSan
 * (tests/test_row_streams_host.py builds and runs it).  For both group widths (ng 8 = 8-lane groups, ng 4 = 16-lane groups),
 * the row strides 256 .. 1024 and stores of 1-residue sequences only, streams shorter than G - 1 positions, streams of very
 * unequal length in one wave slot and a spread of ordinary lengths:
 *   - the layout formula: position p of stream s sits at tok_off[s] + 16 (s + 1) + p, and the array is tok plus 16 per stream;
 *   - the front pad (16 positions of NOP's row) and the tail pad (NOP's row to the padded end);
 *   - the value at EVERY position: code x stride, SEP and NOP included;
 *   - the window bound: every 16-position window the kernel loads -- positions [16 b - lig, 16 b - lig + 15], lig = 0..G-1,
 *     b = 0..nblk + 1 -- lies inside its own stream's region, and holds the stream's codes (NOP in front of position 0);
 *   - a token array whose padding does not cover the lookahead is refused.
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

static Store lay_out(const std::vector<int32_t> &lens, unsigned seed)
{
	Store s;
	s.off.push_back(0);
	for (int32_t len : lens) {
		for (int32_t k = 0; k < len; k++) {
			seed = seed * 1664525u + 1013904223u;
			s.codes.push_back((uint8_t)((seed >> 16) % 24u));
		}
		s.codes.push_back((uint8_t)SA_CODE_SEP);
		s.off.push_back((int32_t)s.codes.size());
	}
	return s;
}

static void check(const char *name, const std::vector<int32_t> &lens, const SaArrKey &key, uint32_t stride)
{
	const int32_t num = (int32_t)lens.size();
	const Store st = lay_out(lens, 7u + stride);
	SaTokenStreams ts;
	std::vector<uint32_t> rows;
	if (!sa_build_tokens(st.codes.data(), st.off.data(), num, key, ts) || !sa_build_row_streams(ts, key.ng, stride, rows)) {
		CHECK(false, "%s: builder failed: %s", name, sa_last_error());
		return;
	}
	const int ng = key.ng, ch = key.ch, g = 64 / ng;
	const int32_t streams = ts.streams;
	CHECK(streams > 0 && streams == num / key.block * (key.block / ch), "%s: %d streams", name, streams);
	CHECK(rows.size() == ts.tok.size() + 16 * (size_t)streams, "%s: %zu row offsets for %zu tokens in %d streams", name, rows.size(),
	      ts.tok.size(), streams);
	if (rows.size() != ts.tok.size() + 16 * (size_t)streams)
		return;
	const uint32_t nop = (uint32_t)SA_CODE_NOP * stride, sep = (uint32_t)SA_CODE_SEP * stride;
	for (int32_t s = 0; s < streams; s++) {
		const int32_t at = ts.tok_off[(size_t)s], padded = ts.tok_off[(size_t)s + 1] - at;
		/* the layout formula, spelled out (not through the header's helper) */
		const int64_t p0 = (int64_t)at + 16 * ((int64_t)s + 1);
		CHECK(sa_row_stream_at(at, s) == p0, "%s: stream %d: position 0 at %lld, expected %lld", name, s, (long long)sa_row_stream_at(at, s), (long long)p0);
		const int64_t lo = p0 - 16, hi = p0 + padded; /* the stream's region: front pad, stream, tail pad */
		CHECK(lo >= 0 && hi <= (int64_t)rows.size(), "%s: stream %d: region [%lld, %lld) of %zu", name, s, (long long)lo, (long long)hi, rows.size());
		if (lo < 0 || hi > (int64_t)rows.size())
			return;
		/* naive stream: its sequences' codes, SEP behind each, NOP before position 0 and from the end on */
		std::vector<uint32_t> naive;
		for (int32_t p = s * ch; p < (s + 1) * ch; p++) {
			for (int32_t k = st.off[(size_t)p]; k < st.off[(size_t)p + 1] - 1; k++)
				naive.push_back((uint32_t)st.codes[(size_t)k] * stride);
			naive.push_back(sep);
		}
		const int32_t slen = (int32_t)naive.size();
		auto want = [&](int32_t p) -> uint32_t { return p >= 0 && p < slen ? naive[(size_t)p] : nop; };
		for (int32_t p = -16; p < padded; p++)
			CHECK(rows[(size_t)(p0 + p)] == want(p), "%s: stream %d position %d: offset %u, expected %u", name, s, p, rows[(size_t)(p0 + p)], want(p));
		for (int32_t p = -16; p < 0; p++)
			CHECK(rows[(size_t)(p0 + p)] == nop, "%s: stream %d: front pad position %d is %u", name, s, p, rows[(size_t)(p0 + p)]);
		for (int32_t p = slen; p < padded; p++)
			CHECK(rows[(size_t)(p0 + p)] == nop, "%s: stream %d: tail pad position %d is %u", name, s, p, rows[(size_t)(p0 + p)]);
		/* the windows of the kernel: the wave slot runs nblk blocks for its longest stream */
		int32_t smax = 0;
		for (int k = s / ng * ng; k < (s / ng + 1) * ng; k++)
			smax = std::max(smax, st.off[(size_t)(k + 1) * ch] - st.off[(size_t)k * ch]);
		const int32_t nblk = (smax + g - 1 + 15) / 16;
		for (int lig = 0; lig < g; lig++)
			for (int32_t b = 0; b <= nblk + 1; b++) {
				const int64_t w0 = p0 + 16 * b - lig, w1 = w0 + 15;
				CHECK(w0 >= lo && w1 < hi, "%s: stream %d lane %d block %d: window [%lld, %lld] outside [%lld, %lld)", name, s, lig, b,
				      (long long)w0, (long long)w1, (long long)lo, (long long)hi);
				if (w0 < lo || w1 >= hi)
					continue;
				for (int k = 0; k < 16; k++)
					CHECK(rows[(size_t)(w0 + k)] == want(16 * b - lig + k), "%s: stream %d lane %d block %d step %d", name, s, lig, b, k);
			}
	}
}

int main()
{
	int cases = 0;
	const SaArrKey shapes[] = { { 8, 1, 0 }, { 8, 3, 0 }, { 4, 1, 0 }, { 4, 2, 0 } };
	const uint32_t strides[] = { 256u, 512u, 768u, 1024u };
	for (const SaArrKey &shape : shapes) {
		SaArrKey key = shape;
		key.block = key.ng * key.ch * SA_PK_WPB; /* one workgroup-tile per arranged block */
		const int32_t num = 3 * key.block + 5;   /* three blocks and a tail that gets no streams */
		const int g = 64 / key.ng;
		char name[96];
		std::vector<int32_t> lens((size_t)num);
		for (uint32_t stride : strides) {
			/* (a) 1-residue sequences only: with ch = 1 every stream is 2 positions, far shorter than G - 1 */
			std::fill(lens.begin(), lens.end(), 1);
			snprintf(name, sizeof(name), "ones ng %d ch %d stride %u", key.ng, key.ch, stride);
			check(name, lens, key, stride);
			cases++;
			/* (b) streams shorter than G - 1 beside streams that end exactly on and one past a block: smax + G - 1 = 16, 17, 32, 33 */
			for (int32_t k = 0; k < num; k++) {
				static const int32_t tot[] = { 16, 17, 32, 33 };
				const int32_t slot = k / (key.ng * key.ch), smax = tot[slot % 4] - (g - 1); /* positions of the slot's longest stream */
				const bool first = k % (key.ng * key.ch) < key.ch;                          /* the slot's first stream is the long one */
				int32_t l = 1;
				if (first && k % key.ch == 0)
					l = std::max(1, smax - 2 * (key.ch - 1) - 1);
				lens[(size_t)k] = l;
			}
			snprintf(name, sizeof(name), "short beside long ng %d ch %d stride %u", key.ng, key.ch, stride);
			check(name, lens, key, stride);
			cases++;
			/* (c) a spread, with a 190 beside 1s in one slot */
			unsigned seed = 99u + (unsigned)key.ch;
			static const int32_t edge[] = { 1, 15, 16, 17, 1, 190, 1, 1, 31, 32, 33, 47, 48, 49, 2, 120 };
			for (int32_t k = 0; k < num; k++) {
				seed = seed * 1664525u + 1013904223u;
				lens[(size_t)k] = k % 3 == 0 ? edge[(size_t)(k / 3) % 16] : 1 + (int32_t)((seed >> 16) % 40u);
			}
			snprintf(name, sizeof(name), "spread ng %d ch %d stride %u", key.ng, key.ch, stride);
			check(name, lens, key, stride);
			cases++;
		}
		/* (d) nothing to build, and a token array whose padding is a block short of the lookahead */
		SaTokenStreams none;
		std::vector<uint32_t> rows(3, 1u);
		CHECK(sa_build_row_streams(none, key.ng, 256u, rows) && rows.empty(), "no streams: %zu offsets", rows.size());
		SaTokenStreams bad;
		bad.streams = key.ng;
		bad.tok_off.resize((size_t)key.ng + 1);
		for (int s = 0; s <= key.ng; s++)
			bad.tok_off[(size_t)s] = 32 * s; /* 32 positions: nblk = 0 */
		bad.tok.assign((size_t)(32 * key.ng), (uint16_t)SA_CODE_NOP);
		CHECK(!sa_build_row_streams(bad, key.ng, 256u, rows), "a stream of 32 padded positions was accepted");
		cases++;
	}
	if (failures) {
		fprintf(stderr, "%d check(s) failed\n", failures);
		return 1;
	}
	printf("ok %d\n", cases);
	return 0;
}
