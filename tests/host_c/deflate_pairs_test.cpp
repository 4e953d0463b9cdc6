/* tests/host_c/deflate_pairs_test.cpp -- the pair parse of the device-side DEFLATE encoder (levels SA_Z_PAIR_LEVEL .. 9,
 * sequencealigner_amd/csrc/sa_deflate_core.h) restated serially on the host: a tile of int32 elements is cut into segments
 * as the kernels cut it, the match finder goes over every segment with the SAME functions and the same order of events
 * (table pre-rolled with the window before the segment, sub-blocks that look up before they insert, the latest position
 * wins, the two claim rounds, every segment counted both ways and left to the fixed parse where pairs do not pay), then histograms, codes, header and bits as in deflate_core_test.cpp with pair starts and
 * their second halves in place.  The Python test inflates the stream with zlib and compares with the input.
 *
 *   deflate_pairs_test <in.i32> <out.zz> <segment elements> <group> <level>   encode a file of little-endian int32 as ONE
 *                                                                             tile; level < SA_Z_PAIR_LEVEL: the fixed parse
 *   deflate_pairs_test --dist                                                 sa_z_dist_code against RFC 1951's table
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_deflate_core.h"

static int dist_cases()
{
	/* RFC 1951 3.2.5: code, extra bits, first distance */
	static const uint32_t base[30] = { 1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
					   193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
	static const uint32_t extra[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
	for (uint32_t d = 1; d <= 32768; d++) {
		int want = 29;
		while (base[want] > d)
			want--;
		uint32_t xb, xv;
		const uint32_t got = sa_z_dist_code(d, &xb, &xv);
		if (got != (uint32_t)want || xb != extra[want] || xv != d - base[want]) {
			fprintf(stderr, "distance %u: code %u (%u bits, %u), want %d (%u bits, %u)\n", d, got, xb, xv, want, extra[want], d - base[want]);
			return 1;
		}
	}
	for (int j = 1; j <= SA_Z_J; j++) {
		uint32_t xb, xv;
		if (sa_z_dist_code(4u * (uint32_t)j, &xb, &xv) != sa_z_dcode(j) || xb != sa_z_dext_bits(j) || xv != sa_z_dext_val(j)) {
			fprintf(stderr, "distance 4 x %d: the general code and the nibble tables disagree\n", j);
			return 1;
		}
	}
	printf("dist ok\n");
	return 0;
}

/* the match finder over one segment [s0, s0 + n) of the tile e[]: start[s0 + k] = elements back if k starts a pair match */
static void find_pairs(const std::vector<uint32_t> &e, size_t s0, size_t n, std::vector<uint16_t> &start)
{
	const uint32_t base = s0 >= (size_t)SA_Z_PAIR_WINDOW ? (uint32_t)s0 - SA_Z_PAIR_WINDOW : 0u;
	std::vector<uint32_t> table(SA_Z_PAIR_TABLE, 0u), cand(n, 0u);
	auto insert = [&](uint32_t at) {
		uint32_t &slot = table[sa_z_pair_hash(e[at], e[at + 1])];
		if (at - base + 1u > slot)
			slot = at - base + 1u;
	};
	for (uint32_t p = base; p < (uint32_t)s0; p++)
		insert(p);
	for (size_t b0 = 0; b0 < n; b0 += SA_Z_PAIR_SUB) {
		const size_t b1 = b0 + SA_Z_PAIR_SUB < n ? b0 + SA_Z_PAIR_SUB : n;
		for (size_t k = b0; k < b1; k++)
			cand[k] = k + 1 < n ? sa_z_pair_candidate(e.data(), table.data(), base, (uint32_t)(s0 + k), e[s0 + k], e[s0 + k + 1]) : 0u;
		for (size_t k = b0; k < b1; k++)
			if (k + 1 < n)
				insert((uint32_t)(s0 + k));
	}
	for (size_t k = 0; k < n; k++)
		start[s0 + k] = (uint16_t)sa_z_pair_claim((uint32_t)k, k ? cand[k - 1] : 0u, cand[k], k + 1 < n ? cand[k + 1] : 0u);
}

/* the segment [s0, s0 + n) counted both ways (sa_z_parse_cost): does the pair parse make it smaller? */
static bool pairs_pay(const std::vector<uint32_t> &e, size_t s0, size_t n, const std::vector<uint16_t> &start)
{
	uint32_t hist[2][320] = {}, extra[2] = {}; /* [0]: the pair parse, [1]: the fixed parse */
	const uint32_t *el = e.data() + s0;
	for (size_t k = 0; k < n; k++) {
		const bool second = k && start[s0 + k - 1], starts = !second && start[s0 + k];
		if (starts) {
			uint32_t xb, xv;
			hist[0][SA_Z_LEN8]++;
			hist[0][288 + sa_z_dist_code(4u * start[s0 + k], &xb, &xv)]++;
			extra[0] += xb;
		}
		const int j = sa_z_match(el, (uint32_t)k);
		for (int w = second || starts ? 1 : 0; w < 2; w++) {
			hist[w][el[k] & 255]++;
			if (j) {
				hist[w][SA_Z_LEN3]++;
				hist[w][288 + sa_z_dcode(j)]++;
				extra[w] += sa_z_dext_bits(j);
			} else {
				for (int t = 1; t < 4; t++)
					hist[w][(el[k] >> (8 * t)) & 255]++;
			}
		}
	}
	uint64_t cost[2];
	for (int w = 0; w < 2; w++) {
		uint32_t lit = 0, dist = 0;
		for (int s = 0; s < 288; s++)
			lit += hist[w][s];
		for (int s = 288; s < 320; s++)
			dist += hist[w][s];
		cost[w] = sa_z_parse_cost(hist[w], lit, hist[w] + 288, dist, extra[w]);
	}
	return cost[0] < cost[1];
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--dist"))
		return dist_cases();
	if (argc != 6) {
		fprintf(stderr, "usage: %s in.i32 out.zz segment_elements segments_per_code_group level | --dist\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	std::vector<uint32_t> e((size_t)bytes / 4);
	if (fread(e.data(), 4, e.size(), f) != e.size())
		return 2;
	fclose(f);
	const size_t seg = (size_t)atol(argv[3]), group = (size_t)atol(argv[4]);
	const bool pairs = atoi(argv[5]) >= SA_Z_PAIR_LEVEL;

	std::vector<uint16_t> start(e.size(), 0);
	size_t claimed = 0, in_pairs = 0; /* elements the finder put inside pair matches; those of segments that kept them */
	if (pairs) {
		for (size_t s0 = 0; s0 < e.size(); s0 += seg) {
			const size_t n = s0 + seg <= e.size() ? seg : e.size() - s0;
			find_pairs(e, s0, n, start);
			size_t here = 0;
			for (size_t k = s0; k < s0 + n; k++) {
				if (!start[k])
					continue;
				here += 2;
				/* a match lies in one segment, inside the window, on equal elements, and shares no element with another */
				if (k + 1 >= s0 + n || start[k] > k || start[k] > SA_Z_PAIR_WINDOW || start[k + 1] || e[k - start[k]] != e[k] ||
				    e[k - start[k] + 1] != e[k + 1]) {
					fprintf(stderr, "element %zu: bad pair match (%u back)\n", k, start[k]);
					return 1;
				}
			}
			claimed += here;
			if (pairs_pay(e, s0, n, start))
				in_pairs += here;
			else
				std::fill(start.begin() + (long)s0, start.begin() + (long)(s0 + n), (uint16_t)0);
		}
	}

	std::vector<uint8_t> out;
	out.push_back(0x78);
	out.push_back(0x9c);
	uint32_t a = 1, b = 0;
	SaZWork W;
	for (size_t g0 = 0; g0 < e.size(); g0 += seg * group) {
		const size_t gend = g0 + seg * group < e.size() ? g0 + seg * group : e.size();
		memset(&W, 0, sizeof(W));
		for (size_t s0 = g0; s0 < gend; s0 += seg) {
			const size_t n = s0 + seg <= gend ? seg : gend - s0;
			const uint32_t *el = e.data() + s0;
			for (size_t k = 0; k < n; k++) {
				if (k && start[s0 + k - 1])
					continue; /* the second half of a pair match */
				if (start[s0 + k]) {
					uint32_t xb, xv;
					W.lfreq[SA_Z_LEN8]++;
					W.dfreq[sa_z_dist_code(4u * start[s0 + k], &xb, &xv)]++;
					continue;
				}
				const uint32_t v = el[k];
				const int j = sa_z_match(el, (uint32_t)k);
				W.lfreq[v & 255]++;
				if (j) {
					W.lfreq[SA_Z_LEN3]++;
					W.dfreq[sa_z_dcode(j)]++;
				} else {
					for (int t = 1; t < 4; t++)
						W.lfreq[(v >> (8 * t)) & 255]++;
				}
			}
			W.lfreq[SA_Z_EOB]++;
		}
		sa_z_alphabet(W, W.lfreq, SA_Z_NLIT, 15, W.llen, W.lcode, 0, false);
		sa_z_alphabet(W, W.dfreq, SA_Z_NDIST, 15, W.dlen, W.dcode, 0, false);
		std::vector<uint32_t> header(256, 0u);
		SaZBits hb{ header.data(), 0 };
		sa_z_header(W, hb, false);
		if (hb.pos > SA_Z_HEADER_BITS) {
			fprintf(stderr, "group at %zu: bad block header (%u bits)\n", g0, hb.pos);
			return 1;
		}
		for (size_t s0 = g0; s0 < gend; s0 += seg) {
			const size_t n = s0 + seg <= gend ? seg : gend - s0;
			const uint32_t *el = e.data() + s0;
			uint64_t s1 = 0, s2 = 0;
			const uint64_t len = 4 * (uint64_t)n;
			std::vector<uint32_t> words(2 * n + 1024, 0u);
			for (size_t k = 0; k < header.size(); k++)
				words[k] = header[k];
			SaZBits bw{ words.data(), hb.pos };
			for (size_t k = 0; k < n; k++) {
				for (int t = 0; t < 4; t++) {
					const uint64_t byte = (el[k] >> (8 * t)) & 255;
					s1 += byte;
					s2 += (len - (4 * k + t)) * byte;
				}
				if (k && start[s0 + k - 1])
					continue;
				uint64_t bits;
				uint32_t nb;
				if (start[s0 + k]) {
					nb = sa_z_pair_bits(W.lcode, W.dcode, start[s0 + k], &bits);
					if (nb > SA_Z_PAIR_BITS)
						return 1;
				} else {
					nb = sa_z_element(W.lcode, W.dcode, el[k], sa_z_match(el, (uint32_t)k), &bits);
				}
				if (nb > SA_Z_ELEM_BITS)
					return 1;
				sa_z_put(bw, (uint32_t)bits, nb > 32 ? 32 : nb);
				if (nb > 32)
					sa_z_put(bw, (uint32_t)(bits >> 32), nb - 32);
			}
			const uint32_t nbytes = sa_z_finish_segment(W.lcode, bw);
			const uint8_t *p = reinterpret_cast<const uint8_t *>(words.data());
			out.insert(out.end(), p, p + nbytes);
			sa_z_adler_append(a, b, (uint32_t)(s1 % 65521u), (uint32_t)(s2 % 65521u), len);
		}
	}
	const uint8_t fin[5] = { 0x01, 0x00, 0x00, 0xff, 0xff };
	out.insert(out.end(), fin, fin + 5);
	const uint32_t adler = b << 16 | a;
	for (int t = 3; t >= 0; t--)
		out.push_back((uint8_t)(adler >> (8 * t)));
	f = fopen(argv[2], "wb");
	if (!f || fwrite(out.data(), 1, out.size(), f) != out.size())
		return 2;
	fclose(f);
	printf("%ld -> %zu bytes (%.3f : 1), %zu of %zu elements inside pair matches (the finder claimed %zu)\n", bytes, out.size(),
	       (double)bytes / (double)out.size(), in_pairs, e.size(), claimed);
	return 0;
}
