/* strands_test.cpp -- the host-compilable core of the two-strand search (csrc/sa_strands_core.h) against plain loops.
 * Built by tests/test_strands_core.py with g++ -fsanitize=address,undefined; every buffer is a heap array of exactly the size the
 * contract gives it, so a write past a row's end or past the bitmap is an ASan report.
 *
 *   --complement        the table: its domain, its pairs, an involution on ATGCSWRYKMBVHDN*, U -> A, 0 elsewhere
 *   --rc                reverse complement of a store: against a plain loop, twice is the identity, the terminators, the refusals
 *                       (which sequence, which position, which byte; no complement / complement not in the scoring's alphabet)
 *   --rule              the segment bounds: multiples of 64, [0, N) once, no more segments than words
 *   --fold N S          fold of rows of N cells cut into S segments for every kind of content (random, all ties, INT32_MIN /
 *                       INT32_MAX cells), with and without raw scores, in place and out of place, with and without the bitmap;
 *                       tail bits zero; then the strand take at pitch k and over a CSR, indices outside [0, N) included
 */
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_strands_core.h"

#define CHECK(cond, ...)                                   \
	do {                                               \
		if (!(cond)) {                             \
			fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
			fprintf(stderr, __VA_ARGS__);      \
			fprintf(stderr, "\n");             \
			exit(1);                           \
		}                                          \
	} while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 32);
}

static const char ALPHABET[] = "ATGCSWRYKMBVHDN*";

static int complement()
{
	uint8_t comp[SA_LUT_SIZE];
	memset(comp, 0xAB, sizeof comp);
	sa_strands_complement_table(comp);
	const char *pairs[] = { "AT", "GC", "RY", "KM", "BV", "HD", "SS", "WW", "NN", "**" };
	for (const char *p : pairs) {
		CHECK(comp[(uint8_t)p[0]] == (uint8_t)p[1], "%c -> %c", p[0], p[1]);
		CHECK(comp[(uint8_t)p[1]] == (uint8_t)p[0], "%c -> %c", p[1], p[0]);
	}
	CHECK(comp[(uint8_t)'U'] == 'A', "U -> A");
	int domain = 0;
	for (int b = 0; b < SA_LUT_SIZE; b++) {
		const bool in = b && (strchr(ALPHABET, b) || b == 'U');
		CHECK((comp[b] != 0) == in, "byte 0x%02x: complement 0x%02x", b, comp[b]);
		domain += in;
		if (in && b != 'U') /* an involution on its domain proper (U leaves it: RNA in, DNA out) */
			CHECK(comp[comp[b]] == b, "involution at %c", b);
		if (in)
			CHECK(strchr(ALPHABET, comp[b]) != nullptr, "the complement of %c is in the alphabet", b);
	}
	CHECK(domain == 17, "17 letters, not %d", domain);
	for (int b = 'a'; b <= 'z'; b++)
		CHECK(comp[b] == 0, "lower case has no complement");
	printf("complement ok\n");
	return 0;
}

struct Store {
	std::vector<uint8_t> blob;
	std::vector<sa_meta> meta;
	sa_input in{};
	explicit Store(const std::vector<std::string> &seqs)
	{
		int32_t max = 0;
		for (const auto &s : seqs) {
			meta.push_back(sa_meta{ (int32_t)blob.size(), (int32_t)s.size() });
			blob.insert(blob.end(), s.begin(), s.end());
			blob.push_back(0);
			max = std::max<int32_t>(max, (int32_t)s.size());
		}
		in.seqs = blob.data();
		in.meta = meta.data();
		in.num = (int32_t)seqs.size();
		in.max = max;
	}
};

static int rc()
{
	uint8_t comp[SA_LUT_SIZE];
	sa_strands_complement_table(comp);
	std::vector<std::string> seqs = { "A", "ACGT", "AACCGGTTN", "RYKMBVHDSWN*", std::string(ALPHABET) };
	for (int len : { 63, 64, 65, 1025 }) {
		std::string s;
		for (int p = 0; p < len; p++)
			s.push_back(ALPHABET[rng() % 16]);
		seqs.push_back(s);
	}
	Store st(seqs);
	int32_t seq = -1, pos = -1;
	uint8_t byte = 0;
	CHECK(sa_strands_rc_check(st.in, comp, nullptr, &seq, &pos, &byte) == SA_RC_OK, "a clean store");
	std::vector<uint8_t> once(st.blob.size(), 0xEE), twice(st.blob.size(), 0xEE);
	sa_strands_rc_write(st.in, comp, once.data());
	for (size_t k = 0; k < seqs.size(); k++) { /* the plain loop */
		const std::string &s = seqs[k];
		for (size_t p = 0; p < s.size(); p++)
			CHECK(once[(size_t)st.meta[k].off + p] == comp[(uint8_t)s[s.size() - 1 - p]], "sequence %zu position %zu", k, p);
		CHECK(once[(size_t)st.meta[k].off + s.size()] == 0, "terminator of %zu", k);
	}
	CHECK(memcmp(once.data() + st.meta[1].off, "ACGT", 5) == 0, "ACGT is its own reverse complement");
	sa_input again = st.in;
	again.seqs = once.data();
	sa_strands_rc_write(again, comp, twice.data());
	CHECK(twice == st.blob, "twice is the identity");
	/* refusals: the FIRST offender, by sequence, position and byte */
	struct Bad {
		size_t k, p;
		char c;
	};
	for (const Bad &b : { Bad{ 0, 0, 'X' }, Bad{ 2, 8, 'a' }, Bad{ 8, 1024, '-' }, Bad{ 3, 5, (char)0xC1 }, Bad{ 4, 0, 'E' } }) {
		std::vector<std::string> bad = seqs;
		bad[b.k][b.p] = b.c;
		if (b.k + 1 < bad.size())
			bad[b.k + 1][0] = '?'; /* a later offender is not the one named */
		Store bs(bad);
		seq = pos = -1;
		byte = 0;
		CHECK(sa_strands_rc_check(bs.in, comp, nullptr, &seq, &pos, &byte) == SA_RC_NO_COMPLEMENT, "no complement for 0x%02x", (uint8_t)b.c);
		CHECK(seq == (int32_t)b.k && pos == (int32_t)b.p && byte == (uint8_t)b.c, "named (%d, %d, 0x%02x), expected (%zu, %zu, 0x%02x)", seq, pos,
		      byte, b.k, b.p, (uint8_t)b.c);
	}
	/* a scoring alphabet without 'Y': R cannot be complemented, Y itself can (its complement R is held) */
	int32_t lut[SA_LUT_SIZE];
	for (int b = 0; b < SA_LUT_SIZE; b++)
		lut[b] = -1;
	for (int t = 0; ALPHABET[t]; t++)
		lut[(uint8_t)ALPHABET[t]] = t;
	lut[(uint8_t)'Y'] = -1;
	Store ys({ "ACGT", "ACYGT", "ACGRT", "R" });
	CHECK(sa_strands_rc_check(ys.in, comp, lut, &seq, &pos, &byte) == SA_RC_NOT_IN_TABLE, "Y is not in the table");
	CHECK(seq == 2 && pos == 3 && byte == 'R', "named (%d, %d, %c)", seq, pos, byte);
	/* U -> A -> T: RNA in, DNA out */
	Store us({ "ACGU" });
	std::vector<uint8_t> uo(us.blob.size());
	sa_strands_rc_write(us.in, comp, uo.data());
	CHECK(memcmp(uo.data(), "ACGT", 5) == 0, "ACGU -> ACGT");
	printf("rc ok\n");
	return 0;
}

static int rule()
{
	CHECK(sa_strand_words(1) == 1 && sa_strand_words(64) == 1 && sa_strand_words(65) == 2 && sa_strand_words(INT32_MAX) == (1 << 25), "words");
	CHECK(sa_strand_pick(5, 5) == SA_STRAND_FORWARD && sa_strand_pick(5, 6) == SA_STRAND_REVERSE && sa_strand_pick(6, 5) == SA_STRAND_FORWARD, "pick");
	CHECK(sa_strand_pick(INT32_MIN, INT32_MAX) == SA_STRAND_REVERSE && sa_strand_pick(INT32_MAX, INT32_MIN) == SA_STRAND_FORWARD, "pick at the limits");
	CHECK(sa_strand_pick(INT32_MIN, INT32_MIN) == SA_STRAND_FORWARD && sa_strand_pick(INT32_MAX, INT32_MAX) == SA_STRAND_FORWARD, "ties at the limits");
	for (int32_t nq : { 1, 2, 3, 7, 100, 2047, 2048, 5000 })
		for (int32_t n : { 1, 63, 64, 65, 127, 128, 129, 130, 1000, 4096, 200003, 1 << 20, INT32_MAX }) {
			const int32_t S = sa_strand_segments(n, nq);
			CHECK(S >= 1 && S <= sa_strand_words(n), "S = %d for (%d, %d)", S, n, nq);
			CHECK(sa_strand_seg_begin(n, S, 0) == 0 && sa_strand_seg_begin(n, S, S) == n, "[0, N) for (%d, %d)", n, nq);
			for (int32_t s : { 0, 1, S / 2, S - 1 }) {
				if (s >= S)
					continue;
				const int32_t b = sa_strand_seg_begin(n, S, s), e = sa_strand_seg_begin(n, S, s + 1);
				CHECK(b % 64 == 0 && b < e && e <= n, "segment %d of %d: [%d, %d) for (%d, %d)", s, S, b, e, n, nq);
				CHECK(e == n || e % 64 == 0, "the end of segment %d of %d is a word's", s, S);
			}
		}
	for (int32_t n : { 1, 63, 64, 65, 128, 129, 1000 })
		for (int32_t S = 1; S <= sa_strand_words(n); S++) { /* every cut the words allow */
			int32_t at = 0;
			for (int32_t s = 0; s < S; s++) {
				CHECK(sa_strand_seg_begin(n, S, s) == at || (at == n && sa_strand_seg_begin(n, S, s) == n), "contiguous");
				CHECK(sa_strand_seg_begin(n, S, s) % 64 == 0 || sa_strand_seg_begin(n, S, s) == n, "a multiple of 64");
				at = sa_strand_seg_begin(n, S, s + 1);
			}
			CHECK(at == n, "covers [0, %d)", n);
		}
	printf("rule ok\n");
	return 0;
}

static int32_t cell(int kind)
{
	static const int32_t limits[] = { INT32_MIN, INT32_MAX, INT32_MIN + 1, INT32_MAX - 1, 0, -1, 1 };
	switch (kind) {
	case 0: /* random, few distinct values: many ties */
		return (int32_t)(rng() % 7) - 3;
	case 1: /* all ties */
		return 42;
	case 2: /* the limits */
		return limits[rng() % 7];
	default: /* random, wide */
		return (int32_t)rng();
	}
}

static int fold(int32_t n, int32_t S)
{
	CHECK(n >= 1 && S >= 1 && S <= sa_strand_words(n), "usage: --fold N S with 1 <= S <= words(N)");
	const int32_t rows = 3, words = (int32_t)sa_strand_words(n);
	long combos = 0, reverse = 0;
	for (int kind = 0; kind < 4; kind++) {
		/* heap arrays of exactly the contract's size */
		std::vector<int32_t> vf((size_t)rows * n), vr((size_t)rows * n), sf((size_t)rows * n), sr((size_t)rows * n);
		for (size_t t = 0; t < vf.size(); t++) {
			vf[t] = cell(kind);
			vr[t] = cell(kind);
			sf[t] = (int32_t)rng();
			sr[t] = (int32_t)rng();
		}
		/* the plain loop */
		std::vector<int32_t> want_v(vf.size()), want_s(vf.size());
		std::vector<uint8_t> want_b(vf.size());
		for (size_t t = 0; t < vf.size(); t++) {
			want_b[t] = vr[t] > vf[t];
			want_v[t] = want_b[t] ? vr[t] : vf[t];
			want_s[t] = want_b[t] ? sr[t] : sf[t];
			reverse += want_b[t];
		}
		if (kind == 1)
			for (uint8_t b : want_b)
				CHECK(b == 0, "an all-tie row is all forward");
		for (int scores = 0; scores < 2; scores++)
			for (int in_place = 0; in_place < 2; in_place++)
				for (int with_bits = 0; with_bits < 2; with_bits++) {
					std::vector<int32_t> a = vf, as = sf, ov(vf.size(), 0x5A5A5A5A), os(vf.size(), 0x5A5A5A5A);
					std::vector<uint64_t> bits((size_t)rows * words, ~(uint64_t)0);
					int32_t *vb = in_place ? a.data() : ov.data(), *sb = !scores ? nullptr : in_place ? as.data() : os.data();
					for (int32_t r = 0; r < rows; r++) {
						const size_t at = (size_t)r * n;
						sa_strand_fold_row(a.data() + at, vr.data() + at, scores ? as.data() + at : nullptr, scores ? sr.data() + at : nullptr, n, S,
								   vb + at, sb ? sb + at : nullptr, with_bits ? bits.data() + (size_t)r * words : nullptr);
					}
					for (size_t t = 0; t < vf.size(); t++) {
						CHECK(vb[t] == want_v[t], "value at %zu (kind %d)", t, kind);
						if (scores)
							CHECK(sb[t] == want_s[t], "score at %zu (kind %d)", t, kind);
					}
					if (!in_place)
						CHECK(a == vf && as == sf, "the inputs are unchanged out of place");
					if (!scores)
						CHECK(as == sf && os == std::vector<int32_t>(vf.size(), 0x5A5A5A5A), "no score is touched without scores");
					if (with_bits)
						for (int32_t r = 0; r < rows; r++) {
							for (int32_t d = 0; d < n; d++)
								CHECK(sa_strand_bit(bits.data() + (size_t)r * words, n, d) == want_b[(size_t)r * n + d], "bit (%d, %d)", r, d);
							for (int32_t d = n; d < words * 64; d++) /* tail bits are zero */
								CHECK(((bits[(size_t)r * words + (d >> 6)] >> (d & 63)) & 1) == 0, "tail bit %d of row %d", d, r);
						}
					else
						for (uint64_t wd : bits)
							CHECK(wd == ~(uint64_t)0, "no bitmap is touched without one");
					combos++;
				}
		/* strand take at pitch k and over a CSR, from the plain loop's bits */
		std::vector<uint64_t> bits((size_t)rows * words, 0);
		for (int32_t r = 0; r < rows; r++)
			for (int32_t d = 0; d < n; d++)
				bits[(size_t)r * words + (d >> 6)] |= (uint64_t)want_b[(size_t)r * n + d] << (d & 63);
		const int32_t k = n < 64 ? n : 64;
		std::vector<int32_t> index((size_t)rows * k);
		for (auto &x : index)
			x = (int32_t)(rng() % (uint32_t)n);
		index[0] = -1;
		index[index.size() - 1] = n;
		if (index.size() > 2)
			index[1] = INT32_MIN;
		std::vector<uint8_t> strand(index.size(), 0x77);
		for (int32_t r = 0; r < rows; r++)
			sa_strand_take_row(bits.data() + (size_t)r * words, n, k, index.data() + (size_t)r * k, strand.data() + (size_t)r * k);
		for (size_t t = 0; t < index.size(); t++) {
			const int32_t d = index[t];
			const uint8_t want = d < 0 || d >= n ? SA_STRAND_NONE : want_b[t / (size_t)k * n + (size_t)d];
			CHECK(strand[t] == want, "strand of hit %zu", t);
		}
		std::vector<int64_t> offsets = { 0, 0, 0, 0 };
		std::vector<int32_t> cidx;
		for (int32_t r = 0; r < rows; r++) {
			if (r != 1) /* (row 1 is empty) */
				for (int32_t d = 0; d < n; d += 1 + (int32_t)(rng() % 3))
					cidx.push_back(d);
			offsets[(size_t)r + 1] = (int64_t)cidx.size();
		}
		std::vector<uint8_t> cst(cidx.size(), 0x77);
		for (int32_t r = 0; r < rows; r++)
			sa_strand_take_csr_row(bits.data() + (size_t)r * words, n, offsets[r], offsets[(size_t)r + 1], cidx.data(), cst.data());
		for (int32_t r = 0; r < rows; r++)
			for (int64_t e = offsets[r]; e < offsets[(size_t)r + 1]; e++)
				CHECK(cst[(size_t)e] == want_b[(size_t)r * n + (size_t)cidx[(size_t)e]], "strand of CSR entry %lld", (long long)e);
	}
	printf("fold ok: N = %d, S = %d, %ld combinations, %ld reverse cells\n", n, S, combos, reverse);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--complement"))
		return complement();
	if (argc == 2 && !strcmp(argv[1], "--rc"))
		return rc();
	if (argc == 2 && !strcmp(argv[1], "--rule"))
		return rule();
	if (argc == 4 && !strcmp(argv[1], "--fold"))
		return fold(atoi(argv[2]), atoi(argv[3]));
	fprintf(stderr, "usage: strands_test --complement | --rc | --rule | --fold N S\n");
	return 2;
}
