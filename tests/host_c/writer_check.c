/* tests/host_c/writer_check.c -- TEST HARNESS: cli/sa_host.c (parsers, HDF5 writer) linked into a plain executable that
 * tests/test_cli_host.py builds with gcc -fsanitize=address,undefined.  Writes a random N x N similarity matrix (packed
 * triangle in, level z) twice -- tiles deflated segment by segment on all cores, and through libhdf5's own filter
 * (SA_HOST_SERIAL_DEFLATE) -- for the test to h5diff.   writer_check <N> <z> <out_parallel.h5> <out_serial.h5>
 * Then the seven side-dataset writers on small arrays into a file of their own beside the first (removed again): each once with
 * valid arguments and once with an argument it refuses, so that the table-driven tail they share runs under the sanitizers too. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cli/sa_host.h"

#define EXPECT(cond) \
	do { \
		if (!(cond)) { \
			fprintf(stderr, "side writers, line %d: %s (%s)\n", __LINE__, #cond, sa_host_error()); \
			return 1; \
		} \
	} while (0)

/* six sequences, k = 2 neighbours each, a graph of four edges, a tree, two quantiles */
static int side_writers(const struct sa_host_store *whole, const char *path)
{
	struct sa_host_store st = *whole;
	st.in.num = 6;
	const int32_t nb_index[12] = { 1, 2, 0, 2, 0, 1, 4, 5, 3, 5, 3, 4 }, nb_score[12] = { 9, 8, 9, 7, 8, 7, 6, 5, 6, 4, 5, 4 };
	struct sa_aln rec[12];
	uint32_t cigar[12];
	for (int t = 0; t < 12; t++) {
		rec[t] = (struct sa_aln){ .score = nb_score[t], .a_end = 4, .b_end = 4, .columns = 4, .identities = 4, .cigar_off = t, .cigar_len = 1 };
		cigar[t] = 4u << 4;
	}
	const int64_t offsets[7] = { 0, 1, 2, 2, 3, 4, 4 }, bad_offsets[7] = { 0, 2, 1, 2, 3, 4, 4 };
	const int32_t eg_index[4] = { 1, 0, 4, 3 }, eg_score[4] = { 9, 9, 6, 6 };
	const int32_t pairs[10] = { 0, 1, 0, 2, 3, 4, 3, 5, 2, 3 }, lk_score[5] = { 9, 8, 6, 5, -3 }, labels[6] = { 0, 0, 0, 3, 3, 3 };
	const int32_t bad_pairs[10] = { 1, 0, 0, 2, 3, 4, 3, 5, 2, 3 };
	const double fractions[2] = { 0.5, 0.9 }, bad_fractions[2] = { 0.5, 1.5 };
	const int32_t values[2] = { 5, 8 }, cut = 8, den[6] = { 20, 20, 20, 20, 20, 20 };
	const int64_t below[2] = { 7, 13 };

	/* the neighbours make the file (create = 1), everything else is added to it */
	EXPECT(sa_host_write_neighbors(path, &st, 2, nb_index, nb_score, 1) == 0);
	EXPECT(sa_host_write_neighbors(path, &st, 6, nb_index, nb_score, 0) != 0 && sa_host_error()[0]);
	EXPECT(sa_host_write_alignments(path, &st, 2, rec, cigar, 12) == 0);
	EXPECT(sa_host_write_alignments(path, &st, 2, rec, NULL, 12) != 0 && sa_host_error()[0]);
	EXPECT(sa_host_write_edges(path, &st, offsets, eg_index, eg_score, 0) == 0);
	EXPECT(sa_host_write_edges(path, &st, bad_offsets, eg_index, eg_score, 0) != 0 && sa_host_error()[0]);
	EXPECT(sa_host_write_linkage(path, &st, pairs, lk_score, labels, 0) == 0);
	EXPECT(sa_host_write_linkage(path, &st, bad_pairs, lk_score, NULL, 0) != 0 && sa_host_error()[0]);
	EXPECT(sa_host_write_quantiles(path, &st, fractions, values, below, 2, &cut, NULL, 0) == 0);
	EXPECT(sa_host_write_quantiles(path, &st, bad_fractions, values, below, 2, NULL, NULL, 0) != 0 && sa_host_error()[0]);
	EXPECT(sa_host_write_normalization(path, &st, den, SA_NORM_SELF, SA_NORM_MIN) == 0);
	EXPECT(sa_host_write_normalization(path, &st, den, 7, SA_NORM_MIN) != 0 && sa_host_error()[0]);
	EXPECT(sa_host_write_identity(path, SA_PID_SHORTER) == 0);
	EXPECT(sa_host_write_identity(path, 9) != 0 && sa_host_error()[0]);
	/* the shared tail's own refusals: a set that is there already, a file that is not */
	EXPECT(sa_host_write_identity(path, SA_PID_SHORTER) != 0 && sa_host_error()[0]);
	remove(path);
	EXPECT(sa_host_write_edges(path, &st, offsets, eg_index, eg_score, 0) != 0 && sa_host_error()[0]);
	/* a graph without edges and a one-sequence tree: sets of extent 0, in files of their own (create = 1) */
	const int64_t none[7] = { 0 };
	EXPECT(sa_host_write_edges(path, &st, none, NULL, NULL, 1) == 0);
	st.in.num = 1;
	EXPECT(sa_host_write_linkage(path, &st, NULL, NULL, NULL, 1) == 0);
	remove(path);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 5)
		return 2;
	const size_t n = (size_t)atol(argv[1]);
	const unsigned z = (unsigned)atoi(argv[2]);
	struct sa_host_store st;
	memset(&st, 0, sizeof(st));
	st.in.num = (int32_t)n;
	st.in.max = 4;
	st.blob_bytes = 5 * n;
	st.in.seqs = malloc(5 * n);
	st.in.meta = malloc(sizeof(*st.in.meta) * n);
	for (size_t k = 0; k < n; k++) {
		memcpy(st.in.seqs + 5 * k, "ARND", 5);
		st.in.meta[k].off = (int32_t)(5 * k);
		st.in.meta[k].len = 4;
	}
	const size_t pairs = n * (n - 1) / 2;
	int32_t *tri = malloc(sizeof(int32_t) * (pairs ? pairs : 1));
	unsigned long long x = 88172645463325252ull;
	for (size_t p = 0; p < pairs; p++) { /* xorshift: scores in [-300, 80) */
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		tri[p] = (int32_t)(x % 380) - 300;
	}
	if (sa_host_write_hdf5(argv[3], &st, tri, true, z)) {
		fprintf(stderr, "%s\n", sa_host_error());
		return 1;
	}
	setenv("SA_HOST_SERIAL_DEFLATE", "1", 1);
	if (sa_host_write_hdf5(argv[4], &st, tri, true, z)) {
		fprintf(stderr, "%s\n", sa_host_error());
		return 1;
	}
	free(tri);
	char side[4096];
	snprintf(side, sizeof(side), "%s.side.h5", argv[3]);
	if (n >= 6 && side_writers(&st, side))
		return 1;
	free(st.in.meta);
	free(st.in.seqs);
	return 0;
}
