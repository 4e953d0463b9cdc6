/*
 * cli/seqalign.c -- the `seqalign` command line tool on top of libseqalign_hip.so.
 *
 * Same surface as the reference binary (src/main.c:9-39 and the per-TU option tables, README "Usage"):
 *   required  -i/--input FILE   -o/--output FILE (or -W)   -m/--matrix NAME   -a/--align METHOD
 *             -p/--gap-penalty N   |   -s/--gap-open N  -e/--gap-extend N
 *   optional  -l/--list-matrices  -f/--filter FLOAT  -z/--compression N  -B/--benchmark  -T/--threads N
 *             -C/--no-cuda  -W/--no-write  -P/--no-progress  -D/--no-detail  -F/--force-proceed
 *             -Q/--quiet  -V/--verbose  -h/--help
 *   added     --column N  --no-header   (non-interactive answers to the reference's DSV column prompt)
 *             -k/--neighbors K  --neighbors-only   (the K best partners of every sequence, selected on the device:
 *             /neighbor_indices and /neighbor_scores; with --neighbors-only no /similarity_matrix at all)
 *             --alignments   (with -k: the N x K pairs (r, neighbor) traced back on the device, records and CIGARs)
 *             --min-score T  --edges-only   (the score graph: every pair that scores at least T as CSR, built on the device:
 *             /edge_offsets, /edge_indices and /edge_scores; with --edges-only no /similarity_matrix at all)
 *             --linkage  --clusters T  --linkage-only   (the single-linkage tree, built on the device: /linkage_pairs and
 *             /linkage_scores; with --clusters also /cluster_labels, the connected components of the pairs that score at least T;
 *             with --linkage-only no /similarity_matrix at all)
 *             --min-quantile Q  --clusters-quantile Q  --quantiles Q1,Q2,...   (the cut as a fraction of the score distribution:
 *             the score at rank min(P - 1, floor(Q P)) of the P pair scores in ascending order, selected on the device by one
 *             sa_*_select call for all of them: /score_quantiles, /score_quantile_values, /score_quantile_below)
 *             --normalize RULE   (everything selected from the scores -- neighbours, score graph, tree, clusters, quantiles -- from
 *             scores divided on the device by the self-scores or the lengths, in parts per million; /similarity_matrix stays raw:
 *             /normalization_denominators, /normalization_rule, /normalization_scale)
 *             --identity DENOM   (the same selections from PERCENT IDENTITY in parts per million: identities of the canonical
 *             alignment of every pair, carried through one sweep on the device, over columns | shorter | longer | mean;
 *             /similarity_matrix stays raw: /identity_rule, /identity_scale)
 * Flow: parse+validate -> load (FASTA/DSV) -> filter -> allocate matrix -> sa_hip_align -> HDF5 -> neighbours -> their alignments -> score graph -> linkage -> -B report.
 * Exit code 1 with a usage hint on any failure (src/main.c:11-14).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <omp.h>
#include <stdarg.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "sa_host.h"

static bool quiet, verbose, force_yes, no_progress;

static void info(const char *fmt, ...)
{
	if (quiet)
		return;
	va_list ap;
	va_start(ap, fmt);
	vprintf(fmt, ap);
	va_end(ap);
	putchar('\n');
}

static void verb(const char *fmt, ...)
{
	if (quiet || !verbose)
		return;
	va_list ap;
	va_start(ap, fmt);
	vprintf(fmt, ap);
	va_end(ap);
	putchar('\n');
}

static void err(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fputs("error: ", stderr);
	vfprintf(stderr, fmt, ap);
	va_end(ap);
	fputc('\n', stderr);
}

/* y/n prompt; -F answers yes (third_party/clix/print.h:585-603), a non-interactive stdin takes the default */
static bool ask(const char *question, bool dflt)
{
	if (force_yes)
		return true;
	if (!isatty(STDIN_FILENO))
		return dflt;
	printf("%s [%s] ", question, dflt ? "Y/n" : "y/N");
	fflush(stdout);
	char line[16];
	if (!fgets(line, sizeof(line), stdin) || line[0] == '\n')
		return dflt;
	return line[0] == 'y' || line[0] == 'Y';
}

static double now(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

struct options {
	const char *input, *output, *matrix, *align;
	long gap_pen, gap_open, gap_ext; /* -1 = not given */
	float filter;
	unsigned compression;
	int threads;
	bool benchmark, no_device, no_write, list;
	int dsv_column, dsv_has_header;
	int neighbors; /* -k: 0 = not given */
	bool neighbors_only;
	bool alignments; /* --alignments: the N x K neighbour pairs traced back */
	bool has_min_score, edges_only; /* --min-score T: the score graph; --edges-only: nothing else */
	int32_t min_score;
	bool linkage, linkage_only, has_clusters; /* --linkage: the single-linkage tree; --clusters T: its labels at T as well */
	int32_t clusters_at;
	/* --min-quantile Q, --clusters-quantile Q, --quantiles Q1,...: the fractions as given, one select call for all of them;
	 * min_q / clusters_q: which of them sets min_score / clusters_at (-1: none) */
	double quantiles[SA_HIP_SELECT_MAX];
	int nquant, min_q, clusters_q;
	/* --normalize RULE: what is selected from the scores is selected from normalised scores (include/seqalign_hip.h: struct sa_norm) */
	bool normalize;
	int32_t norm_source, norm_rule;
	const char *norm_name;
	/* --identity DENOM: what is selected from the scores is selected from percent identity (include/seqalign_hip.h: SA_PID_*) */
	bool identity;
	int32_t pid_denom;
	const char *pid_name;
};

static void usage(const char *argv0)
{
	printf("Usage: %s -i FILE -o FILE -m MATRIX -a METHOD (-p N | -s N -e N) [options]\n"
	       "  -i, --input FILE         Input file path: FASTA, DSV format\n"
	       "  -o, --output FILE        Output file path: HDF5 format\n"
	       "  -m, --matrix MATRIX      Substitution matrix (use -l to list)\n"
	       "  -a, --align METHOD       Needleman-Wunsch: nw | Gotoh: ga | Smith-Waterman: sw\n"
	       "  -p, --gap-penalty N      Linear gap penalty\n"
	       "  -s, --gap-open N         Affine gap open penalty\n"
	       "  -e, --gap-extend N       Affine gap extend penalty\n"
	       "  -l, --list-matrices      List available substitution matrices\n"
	       "  -f, --filter FLOAT       Filter sequences with similarity above threshold [0.0-1.0]\n"
	       "  -z, --compression N      Compression level for HDF5 datasets [0-9]\n"
	       "                           0: none; 1-6: fast parse on the device (between zlib -1 and -4);\n"
	       "                           7-9: smaller files (8-byte pair matches, between zlib -4 and -6)\n"
	       "  -B, --benchmark          Enable timing of various steps\n"
	       "  -T, --threads N          Number of host threads (0 = auto)\n"
	       "  -C, --no-cuda            Not available: this build has no CPU alignment path\n"
	       "  -W, --no-write           Disable writing to output file\n"
	       "  -P, --no-progress        Disable progress bars\n"
	       "  -D, --no-detail          Disable detailed printing (accepted, no-op)\n"
	       "  -F, --force-proceed      Force proceed without user prompts (for CI)\n"
	       "  -Q, --quiet              Suppress all non-error printing\n"
	       "  -V, --verbose            Enable verbose printing\n"
	       "  -k, --neighbors K        Also write the K best partners of every sequence [1-64]:\n"
	       "                           /neighbor_indices and /neighbor_scores (score descending, index ascending)\n"
	       "      --neighbors-only     With -k: no /similarity_matrix, the matrix never leaves the device\n"
	       "      --alignments         With -k: align every sequence with its K neighbors on the device and write\n"
	       "                           /neighbor_alignment_records (N x K x 8: score, a_begin, a_end, b_begin, b_end,\n"
	       "                           columns, identities, cigar_len; a = the sequence, b = its neighbor),\n"
	       "                           /neighbor_cigar_offsets (N*K + 1) and /neighbor_cigars (runs: length << 4 | op,\n"
	       "                           op 0 = M a residue of each, 1 = I of a only, 2 = D of b only)\n"
	       "      --min-score T        Also write the score graph, every pair that scores at least T (any 32-bit integer,\n"
	       "                           negative values included), as CSR over the sequences as written:\n"
	       "                           /edge_offsets (N + 1), /edge_indices and /edge_scores (row r: the entries\n"
	       "                           offsets[r] .. offsets[r + 1], columns ascending)\n"
	       "      --edges-only         With --min-score: no /similarity_matrix, the matrix never leaves the device\n"
	       "                           (not together with -k)\n"
	       "      --linkage            Also write the single-linkage tree (the maximum spanning tree of the scores, built\n"
	       "                           on the device): /linkage_pairs ((N - 1) x 2, lo < hi) and /linkage_scores (N - 1),\n"
	       "                           in the order single linkage joins clusters (score descending)\n"
	       "      --clusters T         The tree, and /cluster_labels (N): the smallest index in each sequence's connected\n"
	       "                           component of the pairs that score at least T (any 32-bit integer)\n"
	       "      --linkage-only       The tree, and no /similarity_matrix: the matrix never leaves the device\n"
	       "                           (not together with -k or --min-score)\n"
	       "      --min-quantile Q     --min-score at T = the score at rank min(P - 1, floor(Q P)) of the P pair scores in\n"
	       "                           ascending order, 0 <= Q <= 1: at least the best (1 - Q) of the pairs (0.99: the best\n"
	       "                           1 %%).  T is selected on the device and written as /edge_min_score; works with\n"
	       "                           --edges-only; not together with --min-score\n"
	       "      --clusters-quantile Q  --clusters at that T, written as /cluster_min_score; works with --linkage-only;\n"
	       "                           not together with --clusters\n"
	       "      --quantiles Q1,Q2,...  Also write the scores at these fractions.  All fractions of the three options\n"
	       "                           (16 at most together) come from one selection: /score_quantiles (the fractions),\n"
	       "                           /score_quantile_values (the scores) and /score_quantile_below (pairs scoring less)\n"
	       "      --normalize RULE     Select from NORMALISED scores: RULE = self-min | self-max | self-mean | len-min |\n"
	       "                           len-max | len-mean.  Every sequence gets a denominator, its self-score (the score of\n"
	       "                           the sequence aligned with itself, computed on the device) or its length; the score s\n"
	       "                           of a pair becomes floor(1000000 s / D), D the smaller, the larger or the mean of the\n"
	       "                           pair's two denominators (parts per million, rounded towards minus infinity; D <= 0\n"
	       "                           gives the lowest value).  Applies to -k, --min-score, --min-quantile, --linkage,\n"
	       "                           --clusters, --clusters-quantile, --quantiles and the --*-only modes, and needs one of\n"
	       "                           them; T of --min-score and --clusters is then in parts per million.\n"
	       "                           /similarity_matrix, when written, STAYS RAW, as does the score of --alignments.\n"
	       "                           Writes /normalization_denominators (N), /normalization_rule (source 0 = self-score,\n"
	       "                           1 = length; rule 0 = min, 1 = max, 2 = mean) and /normalization_scale (1000000)\n"
	       "      --identity DENOM     Select from PERCENT IDENTITY: DENOM = columns | shorter | longer | mean.  Every pair gets\n"
	       "                           the identities of its canonical alignment (the M columns with equal residues of the one\n"
	       "                           alignment --alignments would report), from one sweep on the device with no traceback;\n"
	       "                           its value is floor(1000000 identities / D), D the alignment's columns, the shorter or\n"
	       "                           the longer of the two lengths, or their mean (parts per million; an empty alignment\n"
	       "                           over its columns gives the lowest value).  Applies to -k, --min-score, --min-quantile,\n"
	       "                           --linkage, --clusters, --clusters-quantile, --quantiles and the --*-only modes, and\n"
	       "                           needs one of them; T of --min-score and --clusters is then in parts per million\n"
	       "                           (900000: 90 %% identity).  /similarity_matrix, when written, STAYS RAW.  Not together\n"
	       "                           with --normalize.  Writes /identity_rule (0 = columns, 1 = shorter, 2 = longer,\n"
	       "                           3 = mean) and /identity_scale (1000000)\n"
	       "      --column N           DSV: 1-based sequence column when no header names it\n"
	       "      --no-header          DSV: with --column, the first row is data\n"
	       "  -h, --help               Display this help message\n",
	       argv0);
}

/* a fraction in [0, 1] (no NaN, nothing behind it) onto the list of an option set; false + message otherwise */
struct options;
static bool add_quantile(struct options *o, const char *s, size_t len, int *at);

static bool parse_long(const char *s, long lo, long hi, long *out)
{
	char *end;
	errno = 0;
	const long v = strtol(s, &end, 10);
	if (errno || end == s || *end || v < lo || v > hi)
		return false;
	*out = v;
	return true;
}

static bool add_quantile(struct options *o, const char *s, size_t len, int *at)
{
	char text[64], *end;
	if (len == 0 || len >= sizeof(text)) {
		err("Quantile must be a number between 0 and 1");
		return false;
	}
	memcpy(text, s, len);
	text[len] = 0;
	errno = 0;
	const double q = strtod(text, &end);
	if (errno || end == text || *end || !(q >= 0.0 && q <= 1.0)) {
		err("Quantile must be a number between 0 and 1: %s", text);
		return false;
	}
	if (o->nquant >= SA_HIP_SELECT_MAX) {
		err("At most %d quantiles in all (--min-quantile, --clusters-quantile and --quantiles together)", SA_HIP_SELECT_MAX);
		return false;
	}
	if (at)
		*at = o->nquant;
	o->quantiles[o->nquant++] = q;
	return true;
}

/* returns 0 ok, 1 error, 2 handled-and-exit-success */
static int parse_args(int argc, char **argv, struct options *o)
{
	static const struct {
		const char *lname;
		char sname;
		bool takes;
	} OPTS[] = { { "input", 'i', true }, { "output", 'o', true }, { "matrix", 'm', true }, { "align", 'a', true },
		     { "gap-penalty", 'p', true }, { "gap-open", 's', true }, { "gap-extend", 'e', true },
		     { "list-matrices", 'l', false }, { "filter", 'f', true }, { "compression", 'z', true },
		     { "benchmark", 'B', false }, { "threads", 'T', true }, { "no-cuda", 'C', false },
		     { "no-write", 'W', false }, { "no-progress", 'P', false }, { "no-detail", 'D', false },
		     { "force-proceed", 'F', false }, { "quiet", 'Q', false }, { "verbose", 'V', false },
		     { "help", 'h', false }, { "column", 1, true }, { "no-header", 2, false },
		     { "neighbors", 'k', true }, { "neighbors-only", 3, false }, { "alignments", 4, false },
		     { "min-score", 5, true }, { "edges-only", 6, false }, { "linkage", 7, false }, { "clusters", 8, true },
		     { "linkage-only", 9, false }, { "min-quantile", 10, true }, { "clusters-quantile", 11, true },
		     { "quantiles", 12, true }, { "normalize", 13, true }, { "identity", 14, true },
		     { NULL, 0, false } };
	*o = (struct options){ .gap_pen = -1, .gap_open = -1, .gap_ext = -1, .dsv_column = -1, .dsv_has_header = 1, .min_q = -1, .clusters_q = -1 };
	for (int k = 1; k < argc; k++) {
		const char *arg = argv[k];
		if (arg[0] != '-' || !arg[1]) {
			err("Unexpected argument: %s", arg);
			return 1;
		}
		/* one long option, or a bundle of short ones (-BVW, third_party/clix/args.h:1651-1695) */
		const char *bundle = arg + 1;
		const bool is_long = arg[1] == '-';
		do {
			int idx = -1;
			const char *inline_val = NULL;
			if (is_long) {
				const char *name = arg + 2, *eq = strchr(name, '=');
				const size_t nlen = eq ? (size_t)(eq - name) : strlen(name);
				for (int t = 0; OPTS[t].lname; t++)
					if (strlen(OPTS[t].lname) == nlen && !strncmp(OPTS[t].lname, name, nlen))
						idx = t;
				inline_val = eq ? eq + 1 : NULL;
			} else {
				for (int t = 0; OPTS[t].lname; t++)
					if (OPTS[t].sname == *bundle)
						idx = t;
			}
			if (idx < 0) {
				err("Unknown option: %s", arg);
				return 1;
			}
			const char *val = NULL;
			if (OPTS[idx].takes) {
				if (inline_val)
					val = inline_val;
				else if (!is_long && bundle[1])
					val = bundle + 1; /* -p4 */
				else if (k + 1 < argc)
					val = argv[++k];
				else {
					err("Option --%s requires a parameter", OPTS[idx].lname);
					return 1;
				}
			}
			long v;
			switch (OPTS[idx].sname) {
			case 'i': o->input = val; break;
			case 'o': o->output = val; break;
			case 'm': o->matrix = val; break;
			case 'a': o->align = val; break;
			case 'p':
			case 's':
			case 'e':
				/* src/bio/align.c:127-128 */
				if (!parse_long(val, 0, INT32_MAX, &v)) {
					err("Gap values must be positive integers");
					return 1;
				}
				*(OPTS[idx].sname == 'p' ? &o->gap_pen : OPTS[idx].sname == 's' ? &o->gap_open : &o->gap_ext) = v;
				break;
			case 'l': o->list = true; break;
			case 'f': {
				char *end;
				o->filter = strtof(val, &end);
				if (end == val || *end || o->filter < 0.0f || o->filter > 1.0f) {
					err("Filter threshold must be between 0.0 and 1.0");
					return 1;
				}
				break;
			}
			case 'z':
				if (!parse_long(val, 0, 9, &v)) {
					err("Compression level must be between 0-9");
					return 1;
				}
				o->compression = (unsigned)v;
				break;
			case 'B': o->benchmark = true; break;
			case 'T':
				if (!parse_long(val, 0, 1024, &v)) {
					err("Invalid thread count");
					return 1;
				}
				o->threads = (int)v;
				break;
			case 'C': o->no_device = true; break;
			case 'W': o->no_write = true; break;
			case 'P': no_progress = true; break;
			case 'D': break;
			case 'F': force_yes = true; break;
			case 'Q': quiet = true; break;
			case 'V': verbose = true; break;
			case 'h': usage(argv[0]); return 2;
			case 1:
				if (!parse_long(val, 1, 1 << 20, &v)) {
					err("Invalid column number");
					return 1;
				}
				o->dsv_column = (int)v - 1;
				break;
			case 2: o->dsv_has_header = 0; break;
			case 'k':
				if (!parse_long(val, 1, SA_HIP_NEIGHBORS_MAX, &v)) {
					err("Neighbor count must be between 1-%d", SA_HIP_NEIGHBORS_MAX);
					return 1;
				}
				o->neighbors = (int)v;
				break;
			case 3: o->neighbors_only = true; break;
			case 4: o->alignments = true; break;
			case 5:
				if (!parse_long(val, INT32_MIN, INT32_MAX, &v)) {
					err("Minimum score must be an integer between %d and %d", INT32_MIN, INT32_MAX);
					return 1;
				}
				o->has_min_score = true;
				o->min_score = (int32_t)v;
				break;
			case 6: o->edges_only = true; break;
			case 7: o->linkage = true; break;
			case 8:
				if (!parse_long(val, INT32_MIN, INT32_MAX, &v)) {
					err("Cluster score must be an integer between %d and %d", INT32_MIN, INT32_MAX);
					return 1;
				}
				o->linkage = o->has_clusters = true;
				o->clusters_at = (int32_t)v;
				break;
			case 9: o->linkage = o->linkage_only = true; break;
			case 10:
				if (o->min_q >= 0) {
					err("Option --min-quantile given twice");
					return 1;
				}
				if (!add_quantile(o, val, strlen(val), &o->min_q))
					return 1;
				break;
			case 11:
				if (o->clusters_q >= 0) {
					err("Option --clusters-quantile given twice");
					return 1;
				}
				if (!add_quantile(o, val, strlen(val), &o->clusters_q))
					return 1;
				o->linkage = true;
				break;
			case 12:
				for (const char *p = val;;) {
					const char *comma = strchr(p, ',');
					if (!add_quantile(o, p, comma ? (size_t)(comma - p) : strlen(p), NULL))
						return 1;
					if (!comma)
						break;
					p = comma + 1;
				}
				break;
			case 13: {
				static const struct {
					const char *name;
					int32_t source, rule;
				} RULES[] = { { "self-min", SA_NORM_SELF, SA_NORM_MIN }, { "self-max", SA_NORM_SELF, SA_NORM_MAX },
					      { "self-mean", SA_NORM_SELF, SA_NORM_MEAN }, { "len-min", SA_NORM_LENGTH, SA_NORM_MIN },
					      { "len-max", SA_NORM_LENGTH, SA_NORM_MAX }, { "len-mean", SA_NORM_LENGTH, SA_NORM_MEAN } };
				o->normalize = false;
				for (size_t t = 0; t < sizeof(RULES) / sizeof(RULES[0]); t++)
					if (!strcmp(val, RULES[t].name)) {
						o->normalize = true;
						o->norm_source = RULES[t].source;
						o->norm_rule = RULES[t].rule;
						o->norm_name = RULES[t].name;
					}
				if (!o->normalize) {
					err("Normalization rule must be one of self-min, self-max, self-mean, len-min, len-max, len-mean: %s", val);
					return 1;
				}
				break;
			}
			case 14: {
				static const struct {
					const char *name;
					int32_t denom;
				} DENOMS[] = { { "columns", SA_PID_COLUMNS }, { "shorter", SA_PID_SHORTER }, { "longer", SA_PID_LONGER }, { "mean", SA_PID_MEAN } };
				o->identity = false;
				for (size_t t = 0; t < sizeof(DENOMS) / sizeof(DENOMS[0]); t++)
					if (!strcmp(val, DENOMS[t].name)) {
						o->identity = true;
						o->pid_denom = DENOMS[t].denom;
						o->pid_name = DENOMS[t].name;
					}
				if (!o->identity) {
					err("Identity denominator must be one of columns, shorter, longer, mean: %s", val);
					return 1;
				}
				break;
			}
			}
			if (is_long || OPTS[idx].takes)
				break;
		} while (*++bundle);
	}
	return 0;
}

/* SA_CLI_TIMES=1 (diagnostics): wall-clock stamps of the tool's stages on stderr */
static double t_process0;
static void stamp(const char *what)
{
	static int on = -1;
	if (on < 0)
		on = getenv("SA_CLI_TIMES") != NULL;
	if (on)
		fprintf(stderr, "[cli %8.1f ms] %s\n", (now() - t_process0) * 1e3, what);
}

static void progress_line(double fraction, void *user)
{
	(void)user;
	fprintf(stderr, "\rAligning sequences: %3d%%", (int)(fraction * 100.0));
	fflush(stderr);
}

/* the tiles of the device walk as they arrive (sa_zjob_next), with the progress line fed from them: tile (r, c) of shell
 * b = max(r, c) arrives when column block b is aligned, and the pairs up to there are (b + 1)^2 of nc^2 */
struct tile_feed {
	sa_zjob *job;
	size_t nc;
	bool show;
};
static int next_tiles(void *user, uint32_t *rows, uint32_t *cols, const uint8_t **streams, size_t *sizes)
{
	struct tile_feed *f = user;
	const int n = sa_zjob_next(f->job, rows, cols, streams, sizes);
	if (n > 0 && f->show) {
		const uint32_t b = rows[n - 1] > cols[n - 1] ? rows[n - 1] : cols[n - 1];
		progress_line((double)(b + 1) * (double)(b + 1) / ((double)f->nc * (double)f->nc), NULL);
	}
	return n;
}

/* the one-call selections, whichever quantity they select from: pid != NULL percent identity under *pid (the *_pid calls),
 * otherwise the *_norm calls, which with norm == NULL are their namesakes */
static bool sel_neighbors(struct sa_input in, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score, const struct sa_norm *norm,
			  const int32_t *pid)
{
	return pid ? sa_hip_neighbors_pid(in, sc, k, index, score, *pid) : sa_hip_neighbors_norm(in, sc, k, index, score, norm);
}

static sa_edges *sel_edges(struct sa_input in, const struct sa_scoring *sc, int32_t min_score, const struct sa_norm *norm, const int32_t *pid)
{
	return pid ? sa_hip_edges_pid(in, sc, min_score, *pid) : sa_hip_edges_norm(in, sc, min_score, norm);
}

static sa_linkage *sel_linkage(struct sa_input in, const struct sa_scoring *sc, const struct sa_norm *norm, const int32_t *pid)
{
	return pid ? sa_hip_linkage_pid(in, sc, *pid) : sa_hip_linkage_norm(in, sc, norm);
}

static bool sel_select(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below,
		       const struct sa_norm *norm, const int32_t *pid)
{
	return pid ? sa_hip_select_pid(in, sc, ranks, m, value, below, *pid) : sa_hip_select_norm(in, sc, ranks, m, value, below, norm);
}

static sa_edges *sel_edges_at_rank(struct sa_input in, const struct sa_scoring *sc, int64_t rank, int32_t *min_score, int64_t *below,
				   const struct sa_norm *norm, const int32_t *pid)
{
	return pid ? sa_hip_edges_at_rank_pid(in, sc, rank, min_score, below, *pid) : sa_hip_edges_at_rank_norm(in, sc, rank, min_score, below, norm);
}

static sa_linkage *sel_linkage_with_ranks(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m, int32_t *value,
					  int64_t *below, const struct sa_norm *norm, const int32_t *pid)
{
	return pid ? sa_hip_linkage_with_ranks_pid(in, sc, ranks, m, value, below, *pid)
		   : sa_hip_linkage_with_ranks_norm(in, sc, ranks, m, value, below, norm);
}

int main(int argc, char **argv)
{
	t_process0 = now();
	struct options o;
	const int prc = parse_args(argc, argv, &o);
	if (prc == 2)
		return 0;
	struct sa_scoring sc;
	memset(&sc, 0, sizeof(sc));
	bool ok = prc == 0;
	if (ok && o.list) { /* -l: src/bio/matrices.c:27-33 */
		printf("\nListing available substitution matrices\n");
		for (int fam = 0; fam < 2; fam++) {
			printf("\n%s Matrices:\n  ", fam ? "Nucleotide" : "Amino");
			for (int k = 0, col = 0; k < sa_matrix_count(); k++)
				if (sa_matrix_is_nucleotide(k) == fam)
					printf("%-10s%s", sa_matrix_name(k), ++col % 5 ? "" : "\n  ");
			putchar('\n');
		}
		return 0;
	}
	/* ---- validation, in the reference's terms (src/bio/align.c:130-201, ga.c:70-88, output.c:126-148) */
	if (ok && !o.input)
		ok = (err("Missing required option: -i, --input"), false);
	if (ok && !o.matrix)
		ok = (err("Missing required option: -m, --matrix"), false);
	if (ok && !o.align)
		ok = (err("Missing required option: -a, --align"), false);
	if (ok && o.output && o.no_write)
		ok = (err("Options -o, --output and -W, --no-write conflict"), false);
	if (ok && !o.output && !o.no_write)
		ok = (err("Missing required option: -o, --output"), false);
	if (ok && o.neighbors_only && !o.neighbors)
		ok = (err("Option --neighbors-only requires -k, --neighbors"), false);
	if (ok && o.alignments && !o.neighbors)
		ok = (err("Option --alignments requires -k, --neighbors"), false);
	if (ok && o.has_min_score && o.min_q >= 0)
		ok = (err("Options --min-score and --min-quantile conflict: one threshold for the score graph"), false);
	if (ok && o.has_clusters && o.clusters_q >= 0)
		ok = (err("Options --clusters and --clusters-quantile conflict: one threshold for the clusters"), false);
	if (ok && o.min_q >= 0)
		o.has_min_score = true; /* (min_score itself follows from the selection) */
	if (ok && o.clusters_q >= 0)
		o.has_clusters = true;
	if (ok && o.edges_only && !o.has_min_score)
		ok = (err("Option --edges-only requires --min-score or --min-quantile"), false);
	if (ok && o.edges_only && o.neighbors)
		ok = (err("Options --edges-only and -k, --neighbors conflict: the neighbors need a pass of their own (use --min-score without --edges-only)"), false);
	if (ok && o.linkage_only && o.neighbors)
		ok = (err("Options --linkage-only and -k, --neighbors conflict: the neighbors need a pass of their own (use --linkage without --linkage-only)"), false);
	if (ok && o.linkage_only && o.has_min_score)
		ok = (err("Options --linkage-only and --min-score conflict: the score graph needs a pass of its own (use --linkage without --linkage-only)"), false);
	if (ok && o.normalize && !o.neighbors && !o.has_min_score && !o.linkage && !o.nquant)
		ok = (err("Option --normalize requires something selected from the scores: -k, --min-score, --min-quantile, --linkage, --clusters, "
			  "--clusters-quantile or --quantiles (the similarity matrix itself stays raw)"), false);
	if (ok && o.identity && o.normalize)
		ok = (err("Options --identity and --normalize conflict: one quantity to select from"), false);
	if (ok && o.identity && !o.neighbors && !o.has_min_score && !o.linkage && !o.nquant)
		ok = (err("Option --identity requires something selected from the scores: -k, --min-score, --min-quantile, --linkage, --clusters, "
			  "--clusters-quantile or --quantiles (the similarity matrix itself stays raw)"), false);
	if (ok && sa_matrix_load(o.matrix, sc.lut, sc.sub))
		ok = (err("Invalid substitution matrix name"), false);
	if (ok && (sc.method = sa_method_parse(o.align)) < 0)
		ok = (err("Invalid alignment method"), false);
	if (ok && o.gap_pen >= 0 && (o.gap_open >= 0 || o.gap_ext >= 0))
		ok = (err("Options -p and -s/-e conflict"), false);
	if (ok && sa_method_gap_kind(sc.method) == SA_GAP_LINEAR) {
		if (o.gap_open >= 0 || o.gap_ext >= 0)
			ok = (err("Affine gaps cannot be set for non-affine methods"), false);
		else if (o.gap_pen < 0)
			ok = (err("Missing required option: -p, --gap-penalty"), false);
	} else if (ok) {
		if (o.gap_pen >= 0)
			ok = (err("Gap penalty cannot be set for non-linear methods"), false);
		else if (o.gap_open < 0 || o.gap_ext < 0)
			ok = (err("Missing required option: -s, --gap-open and -e, --gap-extend"), false);
	}
	if (ok) {
		sc.gap_pen = o.gap_pen >= 0 ? -(int32_t)o.gap_pen : 0;
		sc.gap_opn = o.gap_open >= 0 ? -(int32_t)o.gap_open : 0;
		sc.gap_ext = o.gap_ext >= 0 ? -(int32_t)o.gap_ext : 0;
		if (sc.method == SA_METHOD_GA && sc.gap_opn == sc.gap_ext &&
		    ask("Equal affine gaps found, switch to Needleman-Wunsch?", true)) {
			sc.method = SA_METHOD_NW;
			sc.gap_pen = sc.gap_opn;
			sc.gap_opn = sc.gap_ext = SA_SCORE_MIN;
		}
	}
	if (ok && o.no_device)
		ok = (err("-C/--no-cuda: this build has no CPU alignment path (HIP device required)"), false);
	if (ok && o.output && access(o.output, F_OK) == 0) {
		if (!ask("Output file already exists. Do you want to DELETE it?", false))
			ok = (err("Output file exists and will not be overwritten"), false);
		else if (remove(o.output) != 0)
			ok = (err("Failed to delete existing output file"), false);
	}
	if (!ok) {
		fprintf(stderr, "Use %s -h, --help for usage information\n", argv[0]);
		return 1;
	}

	/* -T: host threads (validate_threads, src/system/os.c:466-473).  The alignment itself runs on the device; the
	 * host's parallel loops are the triangular->full expansion of the HDF5 writer and the CPU filter */
	if (o.threads > 0)
		omp_set_num_threads(o.threads);

	info("SEQUENCE ALIGNER (MI355X / HIP)");
	info("Input: %s", o.input);
	if (o.output)
		info("Output: %s", o.output);
	info("Matrix: %s", o.matrix);
	info("Method: %s", sa_method_name(sc.method));
	if (sc.method == SA_METHOD_NW)
		info("Gap penalty: %d", sc.gap_pen);
	else
		info("Gap open: %d, extend: %d", sc.gap_opn, sc.gap_ext);
	if (o.filter > 0.0f)
		info("Filter threshold: %.1f%%", (double)o.filter * 100.0);
	if (o.neighbors)
		info("Neighbors: %d per sequence%s", o.neighbors, o.neighbors_only ? " (no similarity matrix)" : "");
	if (o.min_q >= 0)
		info("Score graph: pairs that score at least the %g quantile of the scores%s", o.quantiles[o.min_q],
		     o.edges_only ? " (no similarity matrix)" : "");
	else if (o.has_min_score)
		info("Score graph: pairs that score at least %d%s", o.min_score, o.edges_only ? " (no similarity matrix)" : "");

	if (o.linkage)
		info("Single-linkage tree%s", o.linkage_only ? " (no similarity matrix)" : "");
	if (o.clusters_q >= 0)
		info("Clusters: connected components of the pairs that score at least the %g quantile of the scores", o.quantiles[o.clusters_q]);
	else if (o.has_clusters)
		info("Clusters: connected components of the pairs that score at least %d", o.clusters_at);
	if (o.nquant)
		info("Score quantiles: %d, selected on the device", o.nquant);
	if (o.normalize)
		info("Normalization: %s, in parts per million (the similarity matrix stays raw)", o.norm_name);

	if (o.identity)
		info("Percent identity over %s, in parts per million (the similarity matrix stays raw)", o.pid_name);

	double t_in = 0, t_filter = 0, t_align = 0, t_out = 0, t_select = 0, t_edges = 0, t_linkage = 0, t0;
	stamp("options parsed");
	struct sa_host_store store;
	t0 = now();
	if (sa_host_load(o.input, sc.lut, sc.gap_pen, o.dsv_column, o.dsv_has_header, &store)) {
		err("%s", sa_host_error());
		return 1;
	}
	t_in = now() - t0;
	stamp("input loaded");
	t0 = now();
	const int32_t before = store.in.num;
	if (o.filter > 0.0f) { /* similarity relation on the device, greedy keep/drop in sequence order (filter.c:14-89) */
		uint8_t *keep = malloc((size_t)store.in.num);
		if (!keep || sa_hip_filter(store.in, o.filter, keep) < 0) {
			err("%s", keep ? sa_last_error() : "Out of memory during sequence filtering");
			return 1;
		}
		if (sa_host_compact(&store, keep) < 0) {
			err("%s", sa_host_error());
			return 1;
		}
		free(keep);
	}
	t_filter = now() - t0;
	if (o.filter > 0.0f)
		info("Filtered out %d sequences", before - store.in.num);
	info("Loaded %d sequences", store.in.num);
	info("Average sequence length: %.2f", (double)store.blob_bytes / (double)store.in.num - 1.0);

	if (o.neighbors && (long long)o.neighbors > (long long)store.in.num - 1) {
		err("Neighbor count %d exceeds the %d other sequences", o.neighbors, store.in.num - 1);
		fprintf(stderr, "Use %s -h, --help for usage information\n", argv[0]);
		return 1;
	}
	/* the ranks of the fractions: P is known now.  One select call answers all of them (q_done), where the matrix is */
	int64_t q_ranks[SA_HIP_SELECT_MAX], q_below[SA_HIP_SELECT_MAX];
	int32_t q_values[SA_HIP_SELECT_MAX];
	bool q_done = false, q_second_pass = false;
	double t_quant = 0;
	for (int t = 0; t < o.nquant; t++) {
		q_ranks[t] = sa_score_rank((int64_t)store.in.num * ((int64_t)store.in.num - 1) / 2, o.quantiles[t]);
		if (q_ranks[t] < 0) {
			err("Score quantiles need at least two sequences");
			return 1;
		}
	}
	int32_t *nb_index = NULL, *nb_score = NULL;
	bool nb_done = false, nb_second_pass = false;
	sa_edges *edges = NULL;
	bool eg_second_pass = false;
	sa_linkage *tree = NULL;
	bool lk_second_pass = false;
	int lk_rounds = 0;
	/* --normalize: every selection below goes the normalised way -- the tile job through sa_zjob_normalize, the rest through the
	 * *_norm calls, which with norm == NULL are their namesakes */
	struct sa_norm norm_spec = { o.norm_source, o.norm_rule, NULL };
	const struct sa_norm *norm = NULL;
	double t_norm = 0;
	if (o.normalize) {
		norm_spec.denominators = malloc(sizeof(int32_t) * (size_t)store.in.num);
		if (!norm_spec.denominators) {
			err("Out of memory allocating normalization denominators");
			return 1;
		}
		norm = &norm_spec;
	}
	/* --identity: the same, through sa_zjob_identity and the *_pid calls */
	const int32_t *pid = o.identity ? &o.pid_denom : NULL;
	double t_pid = 0;
	if (o.neighbors) {
		nb_index = malloc(sizeof(int32_t) * (size_t)store.in.num * (size_t)o.neighbors);
		nb_score = malloc(sizeof(int32_t) * (size_t)store.in.num * (size_t)o.neighbors);
		if (!nb_index || !nb_score) {
			err("Out of memory allocating neighbor data");
			return 1;
		}
	}

	/* output_load (src/io/output.c:35-55): a full matrix that exceeds 3/4 of the available RAM goes to temporary
	 * file storage and is stored triangular; so is one the device(s) cannot hold */
	const size_t n = (size_t)store.in.num;
	struct sa_output out = { NULL, NULL, n, false };
	bool pinned = false;
	/* -z on a chunked dataset: the tiles are deflated on the device, from the packed scores where they were computed
	 * (include/seqalign_hip.h: sa_hip_tiles_begin / sa_zjob_next) -- no host matrix at all.  libhdf5's filter in the
	 * one writing thread (what flush_hdf5 leaves to H5Dwrite, src/io/format/hdf5.c:148-194) takes 41 CPU-minutes for config 5.
	 * SA_HOST_CPU_DEFLATE=1 keeps zlib at exactly the level asked for (all cores, sa_host_write_hdf5). */
	const long long npairs = (long long)n * ((long long)n - 1) / 2;
	const size_t zchunk = sa_host_hdf5_chunk_dim(n);
	const bool no_matrix = o.neighbors_only || o.edges_only || o.linkage_only; /* the matrix never leaves the device */
	bool device_deflate = !o.no_write && !no_matrix && n > 256 && !getenv("SA_HOST_MATRIX") &&
			      (o.compression > 0 ? !getenv("SA_HOST_CPU_DEFLATE") && !getenv("SA_HOST_SERIAL_DEFLATE")
						 /* without -z the same walk returns the tiles as they are: H5Dwrite_chunk instead of H5Dwrite's
						  * gather of every tile out of N-wide rows.  On several devices the plain path stays with sa_hip_align
						  * (tiles dealt by DP work, RCCL all-gather: the whole matrix on every device and in host memory);
						  * with -z the walk itself runs on all of them (sa_hip_tiles_begin: block b -> device b mod n) */
						 : sa_hip_device_count() == 1);
	if (device_deflate) {
		/* the packed scores + one tile row: raw, or raw + worst-case slots and streams (1 + 2 x 2.02 x the row's raw bytes); the
		 * pair parse (-z 7..9) keeps two more bytes per element: what its match finder leaves for the encoder */
		const size_t row_raw = ((n + zchunk - 1) / zchunk) * zchunk * zchunk * sizeof(int32_t);
		device_deflate = sa_hip_memory(sizeof(int32_t) * (size_t)npairs + (o.compression ? 6 : 1) * row_raw +
					       (o.compression >= SA_HIP_Z_PAIR_LEVEL ? row_raw / 2 : 0));
		stamp("device memory probed (runtime up)");
	}
	if (!o.no_write && !device_deflate && !no_matrix) {
		const size_t full_bytes = sizeof(int32_t) * n * n;
		const bool tmpf = sa_host_matrix_needs_file(n);
		out.triangular = tmpf || !sa_hip_memory(full_bytes);
		stamp("device memory probed (runtime up)");
		info("Similarity Matrix dimensions: %zu x %zu%s", n, n, out.triangular ? " (stored triangular)" : "");
		if (tmpf)
			info("Similarity Matrix size exceeds memory limits, creating temporary file storage");
		t0 = now();
		out.matrix = sa_host_matrix_alloc(n, out.triangular, tmpf);
		if (!out.matrix) {
			err("%s", sa_host_error());
			return 1;
		}
		stamp("matrix allocated");
		/* page-lock it for the device->host copies while it is being set up (a file-backed matrix is larger than
		 * RAM by definition and stays pageable: the library stages those copies) */
		if (!tmpf) {
			const size_t bytes = sizeof(int32_t) * (out.triangular ? n * (n - 1) / 2 : n * n);
			/* (the library's own rule, sa_ctx_align_host: never lock more than half of what is available -- a
			 * registration of 70 % of free RAM thrashes or meets the OOM killer instead of failing cleanly) */
			const size_t avail = sa_host_available_memory();
			pinned = bytes && (!avail || bytes <= avail / 2) && sa_hip_host_register(out.matrix, bytes) == 0;
		}
		t_out += now() - t0;
		stamp("matrix page-locked");
	}

	const long long pairs = npairs;
	info("Performing %lld pairwise alignments", pairs);
	/* progress (ppercent / pproportc in the reference's launch loop, src/interface/seqalign_cuda.c:181,286-289,293) */
	const bool show_progress = !no_progress && !quiet;
	if (show_progress) {
		sa_hip_set_progress(progress_line, NULL);
		progress_line(0.0, NULL);
	}
	verb("Devices: %d (%s)", sa_hip_device_count(), sa_hip_device_name(0) ? sa_hip_device_name(0) : "none");
	double t_setup = 0;
	int schedule = 0;
	if (device_deflate) {
		info("Similarity Matrix dimensions: %zu x %zu (%s on the device, tile by tile)", n, n, o.compression ? "deflated" : "tiled");
		/* the alignment runs on the device while the finished tiles are written: the tiles whose larger tile index is b
		 * need exactly column block b (include/seqalign_hip.h: sa_hip_tiles_begin).  The reference's phases (src/main.c:31-34,
		 * bench_align / bench_io) overlap here: "Alignment" below is the device's alignment time, "Output" the rest of
		 * the wall time of this section. */
		t0 = now();
		sa_zjob *job = sa_hip_tiles_begin(store.in, &sc, zchunk, (int)o.compression);
		if (!job) {
			err("%s", sa_last_error());
			return 1;
		}
		t_setup = now() - t0;
		stamp("sa_hip_tiles_begin returned");
		t0 = now();
		struct tile_feed feed = { job, sa_zjob_tiles_per_row(job), show_progress };
		if (sa_host_write_hdf5_streams(o.output, &store, o.compression, next_tiles, &feed)) {
			err("%s (%s)", sa_host_error(), sa_last_error());
			return 1;
		}
		if (show_progress) {
			progress_line(1.0, NULL);
			fputc('\n', stderr);
			sa_hip_set_progress(NULL, NULL);
		}
		t_align = sa_zjob_align_seconds(job);
		const double section = now() - t0;
		t_out += section > t_align ? section - t_align : 0.0;
		double enc_ms = 0, copy_ms = 0;
		uint64_t raw = 0, outb = 0;
		sa_zjob_stats(job, &enc_ms, &copy_ms, &raw, &outb);
		verb("%s on the device: %.2f GB -> %.2f GB (%.2f : 1); the writer waited %.0f ms for the encoder, %.0f ms for gather + copy",
		     o.compression ? "Deflated" : "Tiled", (double)raw / 1e9, (double)outb / 1e9, outb ? (double)raw / (double)outb : 0.0, enc_ms,
		     copy_ms);
		/* --normalize: every tile is written, raw; the device's matrix is normalised in place for what is selected from it.  A job
		 * that cannot (the matrix dealt over several jobs) answers nothing below: the second passes take over */
		bool job_answers = true;
		if (norm) {
			if (sa_zjob_normalize(job, norm) == 0) {
				t_norm = sa_hip_last_normalize_seconds();
				verb("Scores normalised in place on the device (the tiles written are raw)");
			} else {
				job_answers = false;
				verb("Normalization: %s", sa_last_error());
			}
		}
		/* --identity: likewise; the device's matrix is overwritten with percent identity by one more sweep */
		if (pid) {
			if (sa_zjob_identity(job, *pid) == 0) {
				t_pid = sa_hip_last_identity_seconds();
				verb("Percent identity in place on the device (the tiles written are raw)");
			} else {
				job_answers = false;
				verb("Identity: %s", sa_last_error());
			}
		}
		/* the finished matrix is still on the device: the neighbours come from it, nothing is aligned twice */
		if (o.neighbors && job_answers) {
			if (sa_zjob_neighbors(job, o.neighbors, nb_index, nb_score) == 0) {
				nb_done = true;
				t_select = sa_hip_last_neighbors_seconds();
				verb("Neighbors selected from the device's finished matrix (no second alignment)");
			} else {
				verb("Neighbors: %s", sa_last_error());
			}
		}
		if (o.nquant && job_answers) { /* first: the cut of what follows */
			if (sa_zjob_select(job, q_ranks, o.nquant, q_values, q_below) == 0) {
				q_done = true;
				t_quant = sa_hip_last_select_seconds();
				if (o.min_q >= 0)
					o.min_score = q_values[o.min_q];
				verb("Score quantiles selected from the device's finished matrix (no second alignment)");
			} else {
				verb("Score quantiles: %s", sa_last_error());
			}
		}
		if (o.has_min_score && (o.min_q < 0 || q_done) && job_answers) {
			edges = sa_zjob_edges(job, o.min_score);
			if (edges) {
				t_edges = sa_hip_last_edges_seconds();
				verb("Score graph built from the device's finished matrix (no second alignment)");
			} else {
				verb("Score graph: %s", sa_last_error());
			}
		}
		if (o.linkage && job_answers) {
			tree = sa_zjob_linkage(job);
			if (tree) {
				t_linkage = sa_hip_last_linkage_seconds();
				lk_rounds = sa_hip_last_linkage_rounds();
				verb("Single-linkage tree built from the device's finished matrix (no second alignment)");
			} else {
				verb("Single-linkage tree: %s", sa_last_error());
			}
		}
		sa_zjob_destroy(job);
		stamp("HDF5 written");
	} else if (o.linkage_only) {
		/* no host matrix, no tiles, no matrix transfer: align into device memory, build the tree there, copy back 12 (N - 1) bytes */
		info("Similarity Matrix stays on the device: the single-linkage tree is built there");
		t0 = now();
		tree = o.nquant ? sel_linkage_with_ranks(store.in, &sc, q_ranks, o.nquant, q_values, q_below, norm, pid) : sel_linkage(store.in, &sc, norm, pid);
		if (!tree) {
			err("%s", sa_last_error());
			return 1;
		}
		if (o.nquant) {
			q_done = true;
			t_quant = sa_hip_last_select_seconds();
		}
		const double call = now() - t0;
		stamp("sa_hip_linkage returned");
		if (show_progress) {
			progress_line(1.0, NULL);
			fputc('\n', stderr);
			sa_hip_set_progress(NULL, NULL);
		}
		t_align = sa_hip_last_align_seconds();
		t_linkage = sa_hip_last_linkage_seconds();
		lk_rounds = sa_hip_last_linkage_rounds();
		t_setup = call > t_align + t_linkage ? call - t_align - t_linkage : 0.0;
	} else if (o.edges_only) {
		/* no host matrix, no tiles, no matrix transfer: align into device memory, build the graph there, copy back 8 N + 8 E bytes */
		if (o.min_q >= 0)
			info("Similarity Matrix stays on the device: the cut and the pairs at or above it are selected there");
		else
			info("Similarity Matrix stays on the device: the pairs that score at least %d are selected there", o.min_score);
		t0 = now();
		if (o.min_q >= 0 && o.nquant == 1) { /* one alignment: the cut and the graph from the same device matrix */
			edges = sel_edges_at_rank(store.in, &sc, q_ranks[0], &q_values[0], &q_below[0], norm, pid);
		} else {
			if (o.nquant) { /* further fractions: one select call for all of them, in a pass of its own */
				if (!sel_select(store.in, &sc, q_ranks, o.nquant, q_values, q_below, norm, pid)) {
					err("%s", sa_last_error());
					return 1;
				}
				q_second_pass = true;
			}
			if (o.min_q >= 0)
				o.min_score = q_values[o.min_q];
			edges = sel_edges(store.in, &sc, o.min_score, norm, pid);
		}
		if (edges && o.nquant) {
			q_done = true;
			t_quant = sa_hip_last_select_seconds();
			if (o.min_q >= 0)
				o.min_score = q_values[o.min_q];
		}
		if (!edges) {
			err("%s", sa_last_error());
			return 1;
		}
		const double call = now() - t0;
		stamp("sa_hip_edges returned");
		if (show_progress) {
			progress_line(1.0, NULL);
			fputc('\n', stderr);
			sa_hip_set_progress(NULL, NULL);
		}
		t_align = sa_hip_last_align_seconds();
		t_edges = sa_hip_last_edges_seconds();
		t_setup = call > t_align + t_edges ? call - t_align - t_edges : 0.0;
	} else if (o.neighbors_only) {
		/* no host matrix, no tiles, no matrix transfer: align into device memory, select there, copy back 2 N K ints */
		info("Similarity Matrix stays on the device: %d neighbors per sequence are selected there", o.neighbors);
		t0 = now();
		if (!sel_neighbors(store.in, &sc, o.neighbors, nb_index, nb_score, norm, pid)) {
			err("%s", sa_last_error());
			return 1;
		}
		const double call = now() - t0;
		stamp("sa_hip_neighbors returned");
		if (show_progress) {
			progress_line(1.0, NULL);
			fputc('\n', stderr);
			sa_hip_set_progress(NULL, NULL);
		}
		nb_done = true;
		t_align = sa_hip_last_align_seconds();
		t_select = sa_hip_last_neighbors_seconds();
		t_setup = call > t_align + t_select ? call - t_align - t_select : 0.0;
	} else {
		t0 = now();
		if (!sa_hip_align(store.in, out, &sc)) {
			err("%s", sa_last_error());
			return 1;
		}
		t_align = now() - t0;
		stamp("sa_hip_align returned");
		if (show_progress) {
			progress_line(1.0, NULL);
			fputc('\n', stderr);
			sa_hip_set_progress(NULL, NULL);
		}
		/* the reference times the launch/copy loop only (bench_align_start..end inside cuda_align,
		 * src/interface/seqalign_cuda.c:182,292): device set-up and uploads are not part of "Alignment" */
		t_setup = t_align - sa_hip_last_align_seconds();
		t_align = sa_hip_last_align_seconds();
		schedule = sa_hip_last_align_path();

		if (!o.no_write) {
			t0 = now();
			if (sa_host_write_hdf5(o.output, &store, out.matrix, out.triangular, o.compression)) {
				err("%s", sa_host_error());
				return 1;
			}
			t_out += now() - t0;
			stamp("HDF5 written");
		}
	}
	if (o.neighbors && !nb_done) {
		/* the other paths (N <= 256, SA_HOST_* switches, -W, several devices, a walk dealt over several jobs) no longer hold
		 * the matrix on one device: a second pass aligns into device memory again and selects there */
		verb("Neighbors: a second alignment pass into device memory (the matrix of the first is not on one device any more)");
		if (!sel_neighbors(store.in, &sc, o.neighbors, nb_index, nb_score, norm, pid)) {
			err("%s", sa_last_error());
			return 1;
		}
		nb_done = nb_second_pass = true;
		t_select = sa_hip_last_neighbors_seconds();
		stamp("sa_hip_neighbors returned");
	}
	if (o.neighbors && !o.no_write) {
		t0 = now();
		if (sa_host_write_neighbors(o.output, &store, o.neighbors, nb_index, nb_score, o.neighbors_only ? 1 : 0)) {
			err("%s", sa_host_error());
			return 1;
		}
		t_out += now() - t0;
		stamp("neighbors written");
	}
	double t_trace = 0.0;
	long long trace_runs = 0;
	if (o.alignments) {
		/* the N x K pairs (r, neighbor_indices[r][t]), row-major: traced back on the device (include/seqalign_hip.h) */
		const size_t np = (size_t)store.in.num * (size_t)o.neighbors;
		int32_t *pa = malloc(sizeof(int32_t) * np);
		if (!pa) {
			err("Out of memory allocating alignment pairs");
			return 1;
		}
		for (size_t t = 0; t < np; t++)
			pa[t] = (int32_t)(t / (size_t)o.neighbors);
		sa_alns *alns = sa_hip_alignments(store.in, &sc, pa, nb_index, (int64_t)np);
		free(pa);
		if (!alns) {
			err("%s", sa_last_error());
			return 1;
		}
		t_trace = sa_hip_last_alignments_seconds(); /* (reported by itself: the Alignment phase stays the all-vs-all scores) */
		stamp("sa_hip_alignments returned");
		int64_t runs = 0;
		const uint32_t *cigar = sa_alns_cigar(alns, &runs);
		trace_runs = (long long)runs;
		if (!o.no_write) {
			t0 = now();
			if (sa_host_write_alignments(o.output, &store, o.neighbors, sa_alns_records(alns), cigar, runs)) {
				err("%s", sa_host_error());
				return 1;
			}
			t_out += now() - t0;
			stamp("alignments written");
		}
		sa_alns_destroy(alns);
	}
	if (o.nquant && !q_done) {
		/* as for the neighbours: the matrix of the first pass is not on one device any more.  With what the cut feeds where one
		 * alignment can serve both, by itself otherwise */
		verb("Score quantiles: a second alignment pass into device memory (the matrix of the first is not on one device any more)");
		bool got;
		if (o.min_q >= 0 && o.nquant == 1 && !edges) {
			edges = sel_edges_at_rank(store.in, &sc, q_ranks[0], &q_values[0], &q_below[0], norm, pid);
			got = edges != NULL;
			if (got) {
				eg_second_pass = true;
				t_edges = sa_hip_last_edges_seconds();
			}
		} else if (o.linkage && !tree) {
			tree = sel_linkage_with_ranks(store.in, &sc, q_ranks, o.nquant, q_values, q_below, norm, pid);
			got = tree != NULL;
			if (got) {
				lk_second_pass = true;
				t_linkage = sa_hip_last_linkage_seconds();
				lk_rounds = sa_hip_last_linkage_rounds();
			}
		} else {
			got = sel_select(store.in, &sc, q_ranks, o.nquant, q_values, q_below, norm, pid);
		}
		if (!got) {
			err("%s", sa_last_error());
			return 1;
		}
		q_done = q_second_pass = true;
		t_quant = sa_hip_last_select_seconds();
		stamp("score quantiles returned");
	}
	if (q_done) {
		if (o.min_q >= 0) {
			o.min_score = q_values[o.min_q];
			info("Score graph: T = %d, the score at rank %lld of %lld: %lld pairs score at least T", o.min_score, (long long)q_ranks[o.min_q],
			     npairs, npairs - (long long)q_below[o.min_q]);
		}
		if (o.clusters_q >= 0) {
			o.clusters_at = q_values[o.clusters_q];
			info("Clusters: T = %d, the score at rank %lld of %lld: %lld pairs score at least T", o.clusters_at,
			     (long long)q_ranks[o.clusters_q], npairs, npairs - (long long)q_below[o.clusters_q]);
		}
	}
	if (o.has_min_score && !edges) {
		/* as for the neighbours: the matrix of the first pass is not on one device any more */
		verb("Score graph: a second alignment pass into device memory (the matrix of the first is not on one device any more)");
		edges = sel_edges(store.in, &sc, o.min_score, norm, pid);
		if (!edges) {
			err("%s", sa_last_error());
			return 1;
		}
		eg_second_pass = true;
		t_edges = sa_hip_last_edges_seconds();
		stamp("sa_hip_edges returned");
	}
	long long edge_count = 0;
	if (edges) {
		int64_t count = 0;
		const int32_t *eg_index = sa_edges_index(edges, &count);
		edge_count = (long long)count;
		if (!o.no_write) {
			t0 = now();
			if (sa_host_write_edges(o.output, &store, sa_edges_offsets(edges, NULL), eg_index, sa_edges_score(edges), o.edges_only ? 1 : 0)) {
				err("%s", sa_host_error());
				return 1;
			}
			t_out += now() - t0;
			stamp("edges written");
		}
		sa_edges_destroy(edges);
	}
	if (o.linkage && !tree) {
		/* as for the neighbours: the matrix of the first pass is not on one device any more */
		verb("Single-linkage tree: a second alignment pass into device memory (the matrix of the first is not on one device any more)");
		tree = sel_linkage(store.in, &sc, norm, pid);
		if (!tree) {
			err("%s", sa_last_error());
			return 1;
		}
		lk_second_pass = true;
		t_linkage = sa_hip_last_linkage_seconds();
		lk_rounds = sa_hip_last_linkage_rounds();
		stamp("sa_hip_linkage returned");
	}
	int32_t lk_merges = 0, cluster_count = 0;
	if (tree) {
		const int32_t *lk_pairs = sa_linkage_pairs(tree, &lk_merges), *lk_score = sa_linkage_score(tree);
		int32_t *labels = NULL;
		if (o.has_clusters) {
			labels = malloc(sizeof(int32_t) * (size_t)store.in.num);
			if (!labels) {
				err("Out of memory allocating cluster labels");
				return 1;
			}
			cluster_count = sa_linkage_labels(lk_pairs, lk_score, store.in.num, o.clusters_at, labels);
			if (cluster_count < 0) {
				err("%s", sa_last_error());
				return 1;
			}
			verb("Clusters: %d at score >= %d", cluster_count, o.clusters_at);
		}
		if (!o.no_write) {
			t0 = now();
			if (sa_host_write_linkage(o.output, &store, lk_pairs, lk_score, labels, o.linkage_only ? 1 : 0)) {
				err("%s", sa_host_error());
				return 1;
			}
			t_out += now() - t0;
			stamp("linkage written");
		}
		free(labels);
		sa_linkage_destroy(tree);
	}
	if (q_done && !o.no_write) {
		/* last: whatever was asked for beside the quantiles has made the file by now */
		t0 = now();
		if (sa_host_write_quantiles(o.output, &store, o.quantiles, q_values, q_below, o.nquant, o.min_q >= 0 ? &o.min_score : NULL,
					    o.clusters_q >= 0 ? &o.clusters_at : NULL, 0)) {
			err("%s", sa_host_error());
			return 1;
		}
		t_out += now() - t0;
		stamp("quantiles written");
	}
	if (norm && !o.no_write) {
		/* last, like the quantiles: the denominators came back with whichever call normalised */
		t0 = now();
		if (sa_host_write_normalization(o.output, &store, norm_spec.denominators, norm_spec.source, norm_spec.rule)) {
			err("%s", sa_host_error());
			return 1;
		}
		t_out += now() - t0;
		stamp("normalization written");
	}
	if (pid && !o.no_write) {
		t0 = now();
		if (sa_host_write_identity(o.output, *pid)) {
			err("%s", sa_host_error());
			return 1;
		}
		t_out += now() - t0;
		stamp("identity rule written");
	}
	if (pid && t_pid == 0)
		t_pid = sa_hip_last_identity_seconds(); /* (the *_pid calls: the last of them) */
	if (norm && t_norm == 0)
		t_norm = sa_hip_last_normalize_seconds(); /* (the *_norm calls: the last of them) */
	if (o.benchmark) { /* -B: src/util/benchmark.c:50-64 */
		const double total = t_in + t_filter + t_align + t_out;
		printf("Timing breakdown:\n  Input: %.3f sec\n  Filter: %.3f sec\n  Alignment: %.3f sec\n  Output: %.3f sec\n"
		       "  Total: %.3f sec\n",
		       t_in, t_filter, t_align, t_out, total);
		printf("  (device set-up and upload, outside the phases as in the reference: %.3f sec)\n", t_setup);
		printf("  (schedule: %s)\n", device_deflate ? (o.compression ? "column blocks into device memory, their tiles deflated on the device and written meanwhile"
								       : "column blocks into device memory, their tiles delivered as HDF5 chunks meanwhile")
				       : o.linkage_only ? "the packed matrix stays in device memory, only the single-linkage tree comes back"
				       : o.edges_only ? "the packed matrix stays in device memory, only the edges come back"
				       : o.neighbors_only ? "the packed matrix stays in device memory, only the neighbors come back"
			       : schedule == 2
					       ? "tiles dealt over the devices, RCCL all-gather of the dense shares, placement on every device"
					       : "every device delivers its slice of the packed index straight into the host matrix");
		if (o.neighbors)
			printf("  (neighbor selection on the device, K = %d: %.6f sec%s)\n", o.neighbors, t_select,
			       nb_second_pass ? ", after a second alignment pass into device memory" : "");
		if (o.alignments)
			printf("  (alignments of the %lld neighbor pairs on the device, fill + walk: %.6f sec, %lld CIGAR runs)\n",
			       (long long)store.in.num * o.neighbors, t_trace, trace_runs);
		if (o.nquant)
			printf("  (Score quantiles on the device: %d ranks of %lld pairs, %.6f sec%s)\n", o.nquant, npairs, t_quant,
			       q_second_pass ? ", after a second alignment pass into device memory" : "");
		if (o.has_min_score)
			printf("  (score graph on the device, min score = %d: %lld edges, %.6f sec%s)\n", o.min_score, edge_count, t_edges,
			       eg_second_pass ? ", after a second alignment pass into device memory" : "");
		if (o.linkage)
			printf("  (single-linkage tree on the device: %d merges, %d rounds, %.6f sec%s)\n", lk_merges, lk_rounds, t_linkage,
			       lk_second_pass ? ", after a second alignment pass into device memory" : "");
		if (o.has_clusters)
			printf("  (clusters at score >= %d: %d)\n", o.clusters_at, cluster_count);
		if (norm)
			printf("  (Normalisation on the device, %s: denominators + sweep over %lld pairs, %.6f sec)\n", o.norm_name, npairs, t_norm);
		if (pid)
			printf("  (Percent identity on the device, over %s: one sweep over %lld pairs, %.6f sec)\n", o.pid_name, npairs, t_pid);
		printf("Alignments per second: %.2f\n", t_align > 0 ? (double)pairs / t_align : 0.0);
	}
	if (pinned)
		sa_hip_host_unregister(out.matrix);
	sa_host_matrix_free(out.matrix, n, out.triangular);
	free(nb_index);
	free(nb_score);
	free(norm_spec.denominators);
	sa_host_store_free(&store);
	stamp("released");
	/* everything is written and closed: leave without the runtime's teardown (device reset, queue and signal
	 * destruction: ~0.15 s that nothing waits for) */
	fflush(NULL);
	if (getenv("SA_CLI_CLEAN_EXIT")) /* (a profiler that writes its files from an exit handler: rocprofv3) */
		return 0;
	_exit(0);
}
