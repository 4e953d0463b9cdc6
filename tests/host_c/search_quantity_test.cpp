/* search_quantity_test.cpp -- the host-compilable core of the search quantities (sequencealigner_amd/csrc/sa_search_quantity_core.h)
 * under ASan / UBSan: piece bounds, the head / vector / tail split, 64-bit offsets, the serial restatement of the rectangle
 * sweep against sa_norm_value_rule element by element, the wave-item mapping of the identity rectangle, the take gather.
 * Built and run by tests/test_search_quantity_core.py.
 *
 *   search_quantity_test --pieces    every element of an nq x N rectangle in exactly one piece, one split lane, for N in
 *                                    {1, 3, 4, 63, 64, 65, 1000, 1027} x nq in {1, 2, 7} and every misalignment 0..3
 *   search_quantity_test --offsets   sa_sq_at / sa_sq_piece at q * N just below and above 2^31 and 2^32
 *   search_quantity_test --sweep     sa_sq_normalize_rect == sa_norm_value_rule for the three rules, out of place and in place,
 *                                    source and destination 0..3 elements off 16-byte alignment, independently; q0 in {0, 2}
 *   search_quantity_test --items     sa_sq_identity_item: w -> (d, N + q0 + r), past 2^31 items
 *   search_quantity_test --take      sa_sq_take against a direct gather, indices outside [0, N) included
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sequencealigner_amd/csrc/sa_search_quantity_core.h"

#define CHECK(c, ...) \
	do { \
		if (!(c)) { \
			fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); \
			fprintf(stderr, __VA_ARGS__); \
			fprintf(stderr, "\n"); \
			exit(1); \
		} \
	} while (0)

static const int32_t NS[] = { 1, 3, 4, 63, 64, 65, 1000, 1027 };
static const int32_t NQS[] = { 1, 2, 7 };

static int do_pieces()
{
	long cases = 0;
	for (int32_t n : NS)
		for (int32_t nq : NQS)
			for (int off_in = 0; off_in < 4; off_in++)
				for (int off_out = 0; off_out < 4; off_out++) {
					std::vector<int> seen((size_t)n * (size_t)nq, 0);
					const int64_t pieces = sa_sq_pieces(n, nq);
					CHECK(pieces == (int64_t)nq * ((n + SA_SQ_PIECE - 1) / SA_SQ_PIECE), "N = %d, nq = %d: %lld pieces", n, nq, (long long)pieces);
					for (int64_t p = 0; p < pieces; p++) {
						int64_t r, d0;
						int32_t len, head, vecs;
						sa_sq_piece(n, p, &r, &d0, &len);
						CHECK(r >= 0 && r < nq && d0 >= 0 && len >= 1 && len <= SA_SQ_PIECE && d0 + len <= n, "piece %lld of N = %d: row %lld [%lld, +%d)",
						      (long long)p, n, (long long)r, (long long)d0, len);
						CHECK(d0 % SA_SQ_PIECE == 0, "piece %lld begins at %lld", (long long)p, (long long)d0);
						const int64_t at = sa_sq_at(n, r, d0);
						const uint64_t a_in = 4 * (uint64_t)(off_in + at) + 4096, a_out = 4 * (uint64_t)(off_out + at) + 8192;
						sa_sq_split(a_in, a_out, len, &head, &vecs);
						CHECK(head >= 0 && vecs >= 0 && head + 4 * vecs <= len, "split of %d: head %d, %d vectors", len, head, vecs);
						if (off_in == off_out) {
							CHECK(head <= 3 && len - head - 4 * vecs <= 3, "aligned alike: head %d, tail %d", head, len - head - 4 * vecs);
							CHECK(vecs == 0 || (a_in + 4 * (uint64_t)head) % 16 == 0, "the body of the source is not 16-byte aligned");
							CHECK(vecs == 0 || (a_out + 4 * (uint64_t)head) % 16 == 0, "the body of the destination is not 16-byte aligned");
							CHECK(vecs <= SA_SQ_PIECE / 4, "%d vectors for %d threads", vecs, SA_SQ_PIECE / 4);
						} else {
							CHECK(head == len && vecs == 0, "aligned differently: head %d of %d, %d vectors", head, len, vecs);
						}
						/* what thread tid touches, as the kernel has it */
						for (int32_t tid = 0; tid < SA_SQ_PIECE / 4; tid++) {
							for (int32_t e = tid; e < head; e += SA_SQ_PIECE / 4)
								seen[(size_t)(at + e)]++;
							if (tid < vecs)
								for (int u = 0; u < 4; u++)
									seen[(size_t)(at + head + 4 * tid + u)]++;
							const int32_t e = head + 4 * vecs + tid;
							if (e < len)
								seen[(size_t)(at + e)]++;
						}
					}
					for (size_t e = 0; e < seen.size(); e++)
						CHECK(seen[e] == 1, "N = %d, nq = %d, offsets %d / %d: element %zu covered %d times", n, nq, off_in, off_out, e, seen[e]);
					cases++;
				}
	printf("pieces ok: %ld cases\n", cases);
	return 0;
}

static int do_offsets()
{
	/* rows whose first element sits just below and above 2^31 and 2^32 */
	const int64_t n = 66000;
	for (int64_t edge : { (int64_t)1 << 31, (int64_t)1 << 32 })
		for (int64_t r : { edge / n - 1, edge / n, edge / n + 1 }) {
			CHECK(sa_sq_at(n, r, 0) == r * n, "row %lld", (long long)r);
			CHECK((sa_sq_at(n, edge / n, 0) <= edge) && (sa_sq_at(n, edge / n + 1, 0) > edge), "the rows do not straddle %lld", (long long)edge);
			const int64_t per_row = sa_sq_pieces_per_row(n);
			for (int64_t c : { (int64_t)0, per_row - 1 }) {
				int64_t rr, d0;
				int32_t len;
				sa_sq_piece(n, r * per_row + c, &rr, &d0, &len);
				CHECK(rr == r && d0 == c * SA_SQ_PIECE && len == (c + 1 < per_row ? SA_SQ_PIECE : (int32_t)(n - d0)), "piece %lld of row %lld", (long long)c,
				      (long long)r);
				CHECK(sa_sq_at(n, rr, d0) == r * n + c * SA_SQ_PIECE && sa_sq_at(n, rr, d0) + len <= (r + 1) * n, "offset of piece %lld of row %lld",
				      (long long)c, (long long)r);
			}
		}
	CHECK(sa_sq_pieces(66000, 32600) == (int64_t)65 * 32600 && sa_sq_at(66000, 32599, 65999) == (int64_t)66000 * 32600 - 1, "the case of the device test");
	CHECK(sa_sq_at(66000, 32599, 65999) > ((int64_t)1 << 31), "past 2^31");
	CHECK(sa_sq_at(INT32_MAX, INT32_MAX - 1, INT32_MAX - 1) == (int64_t)INT32_MAX * INT32_MAX - 1, "the largest rectangle");
	printf("offsets ok\n");
	return 0;
}

static int do_sweep()
{
	std::mt19937_64 rng(20240917u);
	const int32_t special[] = { 0, -5, 1, 7, SA_NORM_PPM, INT32_MAX, INT32_MIN };
	long cases = 0, negative_values = 0;
	for (int32_t n : NS)
		for (int32_t nq : NQS)
			for (int32_t q0 : { 0, 2 })
				for (int off_in = 0; off_in < 4; off_in++)
					for (int off_out = -1; off_out < 4; off_out++) { /* -1: in place */
						const int32_t m = q0 + nq + 1;
						const size_t elems = (size_t)n * (size_t)nq;
						std::vector<int32_t> den((size_t)n + (size_t)m);
						for (size_t t = 0; t < den.size(); t++)
							den[t] = t % 5 == 0 ? special[(t / 5) % 7] : (int32_t)(rng() % 4000) - 100;
						/* 16-byte aligned bases, the views `off` elements in: the split sees real addresses */
						std::vector<int32_t> in_buf(elems + 8), out_buf(elems + 8, 0x5A5A5A5A);
						int32_t *in_base = in_buf.data(), *out_base = out_buf.data();
						while ((uintptr_t)in_base % 16)
							in_base++;
						while ((uintptr_t)out_base % 16)
							out_base++;
						int32_t *in = in_base + off_in, *out = off_out < 0 ? in : out_base + off_out;
						std::vector<int32_t> src(elems);
						for (size_t e = 0; e < elems; e++)
							src[e] = in[e] = e == 0 ? INT32_MIN : e == elems - 1 ? INT32_MAX : (int32_t)(uint32_t)rng();
						for (int32_t rule = 0; rule < 3; rule++) {
							for (size_t e = 0; e < elems; e++)
								in[e] = src[e];
							sa_sq_normalize_rect(in, n, q0, nq, den.data(), rule, out);
							for (int32_t r = 0; r < nq; r++)
								for (int32_t d = 0; d < n; d++) {
									const size_t e = (size_t)r * (size_t)n + (size_t)d;
									const int32_t want = sa_norm_value_rule(src[e], den[(size_t)d], den[(size_t)n + (size_t)q0 + (size_t)r], rule);
									CHECK(out[e] == want, "N = %d, nq = %d, q0 = %d, rule %d, offsets %d / %d: (%d, %d) is %d, expected %d", n, nq, q0, rule,
									      off_in, off_out, r, d, out[e], want);
									negative_values += want < 0 && want > INT32_MIN && src[e] < 0;
								}
							cases++;
						}
					}
	/* (values below zero are among the cases; the rounding rule itself is sa_norm_value_rule's and is tested where that is) */
	CHECK(negative_values > 1000, "only %ld negative values", negative_values);
	printf("sweep ok: %ld cases, %ld negative values\n", cases, negative_values);
	return 0;
}

static int do_items()
{
	for (int32_t n : { 1, 3, 45, 66000 })
		for (int32_t q0 : { 0, 2, 17 }) {
			int64_t w = 0;
			for (int32_t r = 0; r < 5; r++)
				for (int32_t d = 0; d < n; d += (n > 100 ? 997 : 1)) {
					int32_t i, j;
					w = (int64_t)r * n + d;
					sa_sq_identity_item(n, q0, w, &i, &j);
					CHECK(i == d && j == n + q0 + r && i < j, "N = %d, q0 = %d: item %lld is (%d, %d)", n, q0, (long long)w, i, j);
				}
		}
	int32_t i, j;
	sa_sq_identity_item(66000, 3, ((int64_t)1 << 31) + 5, &i, &j);
	CHECK(i == (int32_t)((((int64_t)1 << 31) + 5) % 66000) && j == 66000 + 3 + (int32_t)((((int64_t)1 << 31) + 5) / 66000), "past 2^31: (%d, %d)", i, j);
	printf("items ok\n");
	return 0;
}

static int do_take()
{
	std::mt19937 rng(99u);
	for (int32_t n : { 1, 5, 65, 1027 })
		for (int32_t nq : { 1, 3 })
			for (int32_t k : { 1, 7, 64 }) {
				if (k > n)
					continue;
				std::vector<int32_t> rect((size_t)n * (size_t)nq), index((size_t)nq * (size_t)k), out((size_t)nq * (size_t)k, 0x5A5A5A5A);
				for (auto &v : rect)
					v = (int32_t)rng();
				for (auto &v : index)
					v = (int32_t)(rng() % (unsigned)n);
				index[0] = -1; /* the caller's error: reads nothing */
				index[index.size() - 1] = n;
				sa_sq_take(rect.data(), n, nq, k, index.data(), out.data());
				for (int32_t r = 0; r < nq; r++)
					for (int32_t t = 0; t < k; t++) {
						const size_t h = (size_t)r * (size_t)k + (size_t)t;
						const int32_t d = index[h];
						const int32_t want = d >= 0 && d < n ? rect[(size_t)r * (size_t)n + (size_t)d] : INT32_MIN;
						CHECK(out[h] == want, "N = %d, nq = %d, k = %d: hit (%d, %d) is %d, expected %d", n, nq, k, r, t, out[h], want);
					}
			}
	printf("take ok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--pieces"))
		return do_pieces();
	if (argc == 2 && !strcmp(argv[1], "--offsets"))
		return do_offsets();
	if (argc == 2 && !strcmp(argv[1], "--sweep"))
		return do_sweep();
	if (argc == 2 && !strcmp(argv[1], "--items"))
		return do_items();
	if (argc == 2 && !strcmp(argv[1], "--take"))
		return do_take();
	fprintf(stderr, "usage: search_quantity_test --pieces | --offsets | --sweep | --items | --take\n");
	return 2;
}
