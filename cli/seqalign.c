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
 *             --linkage-method single|complete|average   (which hierarchy that tree is: complete and average linkage are built on the
 *             device from the whole matrix; /linkage_method says which, /cluster_labels are then the clusters merged at T or above)
 *             --min-quantile Q  --clusters-quantile Q  --quantiles Q1,Q2,...   (the cut as a fraction of the score distribution:
 *             the score at rank min(P - 1, floor(Q P)) of the P pair scores in ascending order, selected on the device by one
 *             sa_*_select call for all of them: /score_quantiles, /score_quantile_values, /score_quantile_below)
 *             --normalize RULE   (everything selected from the scores -- neighbours, score graph, tree, clusters, quantiles -- from
 *             scores divided on the device by the self-scores or the lengths, in parts per million; /similarity_matrix stays raw:
 *             /normalization_denominators, /normalization_rule, /normalization_scale)
 *             --identity DENOM   (the same selections from PERCENT IDENTITY in parts per million: identities of the canonical
 *             alignment of every pair, carried through one sweep on the device, over columns | shorter | longer | mean;
 *             /similarity_matrix stays raw: /identity_rule, /identity_scale)
 *             --query FILE  --query-scores   (a search: the sequences of FILE against the input as the database, with -k the K best
 *             database sequences of every query selected on the device: /query_sequences, /hit_indices and /hit_scores, with
 *             --alignments /hit_alignment_records, /hit_cigar_offsets and /hit_cigars, with --query-scores /query_scores; only the
 *             M x N query-database pairs are aligned, no /similarity_matrix)
 *             --hits-by QUANTITY  (with --query: the hits ranked by a normalised score or by percent identity instead of the raw score:
 *             /hit_values beside /hit_indices, /hit_scores the raw score of each hit, /hit_quantity, /hit_scale, the denominators,
 *             with --query-scores /query_values)
 *             --hits-min T  (with --query, in place of -k: every hit whose value is at least T, as CSR: /hitlist_offsets,
 *             /hitlist_indices, /hitlist_scores, /hitlist_min, under --hits-by /hitlist_values, with --alignments
 *             /hitlist_alignment_records, /hitlist_cigar_offsets and /hitlist_cigars)
 *             --strands forward|both  (with --query, both: every query also reverse-complemented, the two searches folded on the device
 *             by the larger value: /hit_strands or /hitlist_strands beside the hits of the folded search, with --query-scores
 *             /query_strands; forward, the default, writes what a run without the option writes)
 *             --fit  (with --query and -k, NW or Gotoh: every query fitted INSIDE the database sequence -- the whole query, the
 *             database's overhang free: /hit_scores are the fit scores, /hit_db_begin and /hit_db_end the span of the database sequence
 *             the query sits in, /search_ends 1; --alignments the fitted alignments)
 * Flow (main, one function per phase): options -> banner -> load + filter -> output plan -> the first pass (tile job | one selection only |
 * host matrix | the search) -> per selection, in the order of the file: its second pass where the first left it unanswered, then its
 * datasets (a search: its alignments, then its one file) -> -B report.
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
	/* --linkage-method NAME: which hierarchy the tree is (0 single, SA_AGGLO_COMPLETE, SA_AGGLO_AVERAGE); without the option:
	 * single, and the output is what it was before the option existed */
	bool has_method;
	int32_t method;
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
	/* --query FILE: a search of FILE's sequences against the input; -k is then the hits per query.  --query-scores: /query_scores too */
	const char *query;
	bool query_scores;
	/* --hits-by QUANTITY: what the hits of a search are ranked by -- kind 0 the score (as without the option), 1 a normalised score
	 * (hits_source, hits_rule), 2 percent identity (hits_denom) */
	bool hits_by;
	int32_t hits_kind, hits_source, hits_rule, hits_denom;
	const char *hits_name;
	/* --hits-min T: with --query, in place of -k: every hit whose value (the quantity of --hits-by, or the raw score) is at least T */
	bool has_hits_min;
	int32_t hits_min;
	/* --strands forward|both: with --query, both: every query is searched as written and reverse-complemented, the two folded on the
	 * device (include/seqalign_hip.h: sa_hip_search_strands); forward, the default: the output of a run without the option */
	bool strands_both;
	/* --fit: with --query and -k: the queries fitted inside the database sequences (include/seqalign_hip.h: sa_hip_search_fit) */
	bool fit;
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
	       "      --linkage-method NAME  The hierarchy of --linkage, --clusters, --clusters-quantile and --linkage-only, and\n"
	       "                           needs one of them: single (the default) | complete | average.  complete: the similarity\n"
	       "                           of two clusters is their LOWEST cross pair, so with --clusters T every pair inside a\n"
	       "                           cluster scores at least T (single linkage promises that of one chain of pairs only);\n"
	       "                           average: the mean of their cross pairs (UPGMA), exact, /linkage_scores its floor.\n"
	       "                           Both are built on the device from the whole matrix, in the order the merges are made\n"
	       "                           (score non-increasing; a cluster is named by its smallest member), and need a square\n"
	       "                           working matrix beside the scores (4 N^2 bytes, average 8 N^2).  /cluster_labels: the\n"
	       "                           smallest index in each sequence's cluster after the merges at T or above.  Writes\n"
	       "                           /linkage_method (0 = single, 1 = complete, 2 = average)\n"
	       "      --min-quantile Q    --min-score at T = the score at rank min(P - 1, floor(Q P)) of the P pair scores in\n"
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
	       "      --query FILE         A search: the M sequences of FILE (same formats, same residue checks) as queries against the\n"
	       "                           N of the input as the database.  Needs -k K, 1 <= K <= min(N, 64) (or --hits-min T\n"
	       "                           instead: every hit at or above a threshold, see there).  Only the M x N\n"
	       "                           query-database pairs are aligned: no all-vs-all, no /similarity_matrix.  Writes\n"
	       "                           /query_sequences (M) beside /sequences, /hit_indices and /hit_scores (M x K: the K best\n"
	       "                           database sequences of every query, score descending, index ascending; indices into\n"
	       "                           /sequences as written, so after -f, which filters the database and never the queries).\n"
	       "                           With --alignments: /hit_alignment_records, /hit_cigar_offsets and /hit_cigars in the\n"
	       "                           format of the neighbor datasets (a = the query, b = its hit).  The database is the row\n"
	       "                           and the query the column sequence of the substitution matrix.  Not together with -z,\n"
	       "                           the --*-only modes or any other selection (--min-score, --min-quantile, --linkage,\n"
	       "                           --clusters, --clusters-quantile, --linkage-method, --quantiles, --normalize, --identity)\n"
	       "      --query-scores       With --query: also /query_scores (M x N), every query-database score\n"
	       "      --hits-by QUANTITY   With --query: rank the hits by QUANTITY = score (as without the option) | self-min |\n"
	       "                           self-max | self-mean | len-min | len-max | len-mean (the normalised scores of --normalize,\n"
	       "                           the denominators those of the database sequence and the query) | identity-columns |\n"
	       "                           identity-shorter | identity-longer | identity-mean (the percent identity of --identity).\n"
	       "                           Values are in parts per million.  Writes /hit_values (M x K, descending, ties by index\n"
	       "                           ascending) beside /hit_indices; /hit_scores is then the raw score of each hit and NO LONGER\n"
	       "                           SORTED.  Also /hit_quantity (kind 1 = normalised, 2 = identity; source or 0; rule or\n"
	       "                           denominator, numbered as /normalization_rule and /identity_rule), /hit_scale (1000000), for\n"
	       "                           the normalised kinds /database_denominators (N) and /query_denominators (M), and with\n"
	       "                           --query-scores /query_values (M x N) beside /query_scores, which stays raw.  --alignments\n"
	       "                           is unchanged (a = the query, b = its hit)\n"
	       "      --hits-min T         With --query, in place of -k (exactly one of the two is given): every database sequence\n"
	       "                           whose value against a query is at least T (any 32-bit integer), however many there are.\n"
	       "                           T is in the unit of --hits-by: the raw score without it, parts per million with it\n"
	       "                           (--hits-by identity-shorter --hits-min 900000: at least 90 %% identity).  Writes the\n"
	       "                           hits as CSR: /hitlist_offsets (M + 1, 64-bit), /hitlist_indices and /hitlist_scores (E,\n"
	       "                           the hits of query q at offsets[q] .. offsets[q + 1], index ASCENDING, not ranked: ranking\n"
	       "                           is what -k is for; the scores raw), /hitlist_min (T), under a quantity /hitlist_values\n"
	       "                           (E) with /hit_quantity, /hit_scale and the denominators as --hits-by writes them; with\n"
	       "                           --alignments /hitlist_alignment_records (E x 8), /hitlist_cigar_offsets (E + 1) and\n"
	       "                           /hitlist_cigars; with --query-scores /query_scores and, under a quantity, /query_values,\n"
	       "                           which cost a second alignment of the rectangle (the hit list does not keep it)\n"
	       "      --strands WHICH      With --query: forward (the default: every query as written) | both: every query is also\n"
	       "                           searched reverse-complemented (IUPAC: A-T, G-C, R-Y, K-M, B-V, H-D; S, W, N, * themselves;\n"
	       "                           U as A) and the two results are folded on the device -- per query and database sequence\n"
	       "                           the strand with the larger value (of --hits-by, or the raw score) wins, the forward one on\n"
	       "                           a tie.  /hit_indices, /hit_scores and /hit_values are those of the folded search;\n"
	       "                           /hit_strands (M x K, 8-bit: 0 forward, 1 reverse) is added, under --hits-min\n"
	       "                           /hitlist_strands (E); --query-scores writes the folded /query_scores and /query_values and\n"
	       "                           adds /query_strands (M x N, 8-bit); --alignments traces every hit on its own strand: for\n"
	       "                           a reverse hit a = the REVERSE COMPLEMENT of the query (position p there is position\n"
	       "                           length - 1 - p of the query as given).  /query_sequences stays the queries as given; -f\n"
	       "                           filters the database only.  Needs a nucleotide matrix and queries of the alphabet above\n"
	       "      --fit                With --query and -k, -a nw or ga: fit every query INSIDE the database sequence -- the whole\n"
	       "                           query is aligned, the residues of the database sequence before and behind it cost nothing\n"
	       "                           (semi-global, \"glocal\": a read inside a long entry, a domain inside a protein).\n"
	       "                           /hit_scores are then the fit scores; /hit_db_begin and /hit_db_end (M x K) give the\n"
	       "                           half-open span of the database sequence the query sits in, /search_ends (1) is 1.\n"
	       "                           --hits-by score | identity-* keeps its datasets (the identity is that of the fitted\n"
	       "                           alignment); --query-scores writes the fit scores (and /query_values); --alignments writes\n"
	       "                           the fitted alignments (a = the query, always whole: a_begin 0, a_end its length; b_begin\n"
	       "                           and b_end the span).  Not together with -a sw (local already), --hits-min, --strands both\n"
	       "                           or the normalised kinds of --hits-by\n"
	       "      --column N           DSV: 1-based sequence column when no header names it\n"
	       "      --no-header          DSV: with --column, the first row is data\n"
	       "  -h, --help               Display this help message\n",
	       argv0);
}

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

/* a fraction in [0, 1] (no NaN, nothing behind it) onto the list of an option set; false + message otherwise */
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
		     { "linkage-method", 15, true }, { "query", 16, true }, { "query-scores", 17, false }, { "hits-by", 18, true },
		     { "hits-min", 19, true }, { "strands", 20, true }, { "fit", 21, false },
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
			case 15: {
				static const char *const METHODS[] = { "single", "complete", "average" }; /* 0, SA_AGGLO_COMPLETE, SA_AGGLO_AVERAGE */
				if (o->has_method) {
					err("Option --linkage-method given twice");
					return 1;
				}
				for (int32_t t = 0; t < 3; t++)
					if (!strcmp(val, METHODS[t])) {
						o->has_method = true;
						o->method = t;
					}
				if (!o->has_method) {
					err("Linkage method must be one of single, complete, average: %s", val);
					return 1;
				}
				break;
			}
			case 19:
				if (!parse_long(val, INT32_MIN, INT32_MAX, &v)) {
					err("Hit threshold must be an integer between %d and %d", INT32_MIN, INT32_MAX);
					return 1;
				}
				o->has_hits_min = true;
				o->hits_min = (int32_t)v;
				break;
			case 20:
				if (strcmp(val, "forward") && strcmp(val, "both")) {
					err("Strands must be one of forward, both: %s", val);
					return 1;
				}
				o->strands_both = !strcmp(val, "both");
				break;
			case 21: o->fit = true; break;
			case 16: o->query = val; break;
			case 17: o->query_scores = true; break;
			case 18: {
				static const struct {
					const char *name;
					int32_t kind, source, rule, denom;
				} BY[] = { { "score", 0, 0, 0, 0 },
					   { "self-min", 1, SA_NORM_SELF, SA_NORM_MIN, 0 }, { "self-max", 1, SA_NORM_SELF, SA_NORM_MAX, 0 },
					   { "self-mean", 1, SA_NORM_SELF, SA_NORM_MEAN, 0 }, { "len-min", 1, SA_NORM_LENGTH, SA_NORM_MIN, 0 },
					   { "len-max", 1, SA_NORM_LENGTH, SA_NORM_MAX, 0 }, { "len-mean", 1, SA_NORM_LENGTH, SA_NORM_MEAN, 0 },
					   { "identity-columns", 2, 0, 0, SA_PID_COLUMNS }, { "identity-shorter", 2, 0, 0, SA_PID_SHORTER },
					   { "identity-longer", 2, 0, 0, SA_PID_LONGER }, { "identity-mean", 2, 0, 0, SA_PID_MEAN } };
				o->hits_by = false;
				for (size_t t = 0; t < sizeof(BY) / sizeof(BY[0]); t++)
					if (!strcmp(val, BY[t].name)) {
						o->hits_by = true;
						o->hits_kind = BY[t].kind;
						o->hits_source = BY[t].source;
						o->hits_rule = BY[t].rule;
						o->hits_denom = BY[t].denom;
						o->hits_name = BY[t].name;
					}
				if (!o->hits_by) {
					err("Hit quantity must be one of score, self-min, self-max, self-mean, len-min, len-max, len-mean, identity-columns, "
					    "identity-shorter, identity-longer, identity-mean: %s", val);
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

/* what is selected from: pid != NULL percent identity under *pid (the *_pid calls, sa_zjob_identity), otherwise norm != NULL
 * normalised scores (the *_norm calls, sa_zjob_normalize), otherwise the scores: the *_norm calls with norm == NULL are their namesakes */
struct quantity {
	const struct sa_norm *norm;
	const int32_t *pid;
};

/* the one-call selections, whichever quantity they select from */
static bool sel_neighbors(struct sa_input in, const struct sa_scoring *sc, int32_t k, int32_t *index, int32_t *score, struct quantity q)
{
	return q.pid ? sa_hip_neighbors_pid(in, sc, k, index, score, *q.pid) : sa_hip_neighbors_norm(in, sc, k, index, score, q.norm);
}

static sa_edges *sel_edges(struct sa_input in, const struct sa_scoring *sc, int32_t min_score, struct quantity q)
{
	return q.pid ? sa_hip_edges_pid(in, sc, min_score, *q.pid) : sa_hip_edges_norm(in, sc, min_score, q.norm);
}

/* (method: 0 the single-linkage tree, otherwise SA_AGGLO_COMPLETE / SA_AGGLO_AVERAGE -- the same result object) */
static sa_linkage *sel_linkage(struct sa_input in, const struct sa_scoring *sc, int32_t method, struct quantity q)
{
	if (method)
		return sa_hip_agglomerate(in, sc, method, q.norm, q.pid);
	return q.pid ? sa_hip_linkage_pid(in, sc, *q.pid) : sa_hip_linkage_norm(in, sc, q.norm);
}

static bool sel_select(struct sa_input in, const struct sa_scoring *sc, const int64_t *ranks, int32_t m, int32_t *value, int64_t *below, struct quantity q)
{
	return q.pid ? sa_hip_select_pid(in, sc, ranks, m, value, below, *q.pid) : sa_hip_select_norm(in, sc, ranks, m, value, below, q.norm);
}

static sa_edges *sel_edges_at_rank(struct sa_input in, const struct sa_scoring *sc, int64_t rank, int32_t *min_score, int64_t *below, struct quantity q)
{
	return q.pid ? sa_hip_edges_at_rank_pid(in, sc, rank, min_score, below, *q.pid) : sa_hip_edges_at_rank_norm(in, sc, rank, min_score, below, q.norm);
}

static sa_linkage *sel_linkage_with_ranks(struct sa_input in, const struct sa_scoring *sc, int32_t method, const int64_t *ranks, int32_t m,
					  int32_t *value, int64_t *below, struct quantity q)
{
	if (method)
		return sa_hip_agglomerate_with_ranks(in, sc, method, q.norm, q.pid, ranks, m, value, below);
	return q.pid ? sa_hip_linkage_with_ranks_pid(in, sc, ranks, m, value, below, *q.pid)
		     : sa_hip_linkage_with_ranks_norm(in, sc, ranks, m, value, below, q.norm);
}

/* One run of the tool: what main's phases hand to each other.  Every selection keeps its result with its bookkeeping: `seconds` the
 * device time of the call that answered it, `second_pass` whether that call aligned again (the -B report says so). */
struct run {
	const char *argv0;
	struct options o;
	struct sa_scoring sc;
	struct sa_host_store store;
	size_t n;
	long long npairs;
	bool show_progress;
	double t_in, t_filter, t_align, t_out, t_setup; /* the phases of the -B report; set-up is outside them, as in the reference */
	int schedule; /* sa_hip_last_align_path of the host-matrix branch */
	struct sa_output out; /* the output plan: the host matrix, or the tile job (device_deflate), or no matrix at all */
	bool pinned, no_matrix, device_deflate;
	size_t zchunk;
	struct sa_norm norm_spec; /* the quantity (--normalize or --identity, never both), and the device time of its sweep */
	struct quantity q;
	double t_quantity;
	double t_write0; /* WRITE_OUT */
	struct { int32_t *index, *score; bool done, second_pass; double seconds; } nb;
	/* --query: the queries, the hits (M x K), with --query-scores the rectangle (M x N), with --alignments the M x K records */
	struct sa_host_store queries;
	struct { int32_t *index, *score, *rect, *value, *vrect, *db_begin, *db_end; sa_alns *alns; double hits_seconds, gather_seconds; int32_t batches; } sr;
	/* --query --hits-min: the hits of every query as CSR (E of them), in arrays the library owns */
	struct { sa_hitlist *list; long long count; double rect_seconds; } ab;
	/* --query --strands both: the strand of every hit (M x K) and, with --query-scores, of every cell (M x N); the device time of
	 * fold + strand take */
	struct { uint8_t *hit, *rect; double seconds; } st;
	struct { double seconds; long long runs; } trace;
	struct { /* the fractions' ranks: one select call answers all of them, where the matrix is */
		int64_t ranks[SA_HIP_SELECT_MAX], below[SA_HIP_SELECT_MAX];
		int32_t values[SA_HIP_SELECT_MAX];
		bool done, second_pass;
		double seconds;
	} qt;
	struct { sa_edges *edges; bool second_pass; double seconds; long long count; } eg;
	struct { sa_linkage *tree; bool second_pass; double seconds; int rounds; long long rescans; int32_t merges, clusters; } lk;
};

/* the tree's name in the messages: "single-linkage", "complete-linkage", "average-linkage"; capital: at the head of a line */
static const char *tree_name(const struct options *o, bool capital)
{
	static const char *const NAMES[3][2] = { { "single-linkage", "Single-linkage" }, { "complete-linkage", "Complete-linkage" },
						 { "average-linkage", "Average-linkage" } };
	return NAMES[o->method][capital ? 1 : 0];
}

static const char *tree_title(const struct options *o)
{
	static const char *const TITLES[3] = { "Single-linkage tree", "Complete-linkage tree", "Average-linkage tree" };
	return TITLES[o->method];
}

/* the end of a phase that cannot go on: the message (sa_last_error(), sa_host_error(), or the tool's own), and false */
static bool failed(const char *message)
{
	err("%s", message);
	return false;
}

/* the end of the progress line, once the alignment is done */
static void finish_progress(const struct run *r)
{
	if (!r->show_progress)
		return;
	progress_line(1.0, NULL);
	fputc('\n', stderr);
	sa_hip_set_progress(NULL, NULL);
}

/* a sa_host_write_* call, unless -W: its message when it failed, otherwise its time to Output and its stamp */
#define WRITE_OUT(r, call, what) ((r)->o.no_write || ((r)->t_write0 = now(), written((r), (call), (what))))
static bool written(struct run *r, int rc, const char *what)
{
	if (rc)
		return failed(sa_host_error());
	r->t_out += now() - r->t_write0;
	stamp(what);
	return true;
}

/* a score graph / a tree as it comes back from whichever call built it (NULL: the call failed, the message is the caller's) */
static bool take_edges(struct run *r, sa_edges *edges)
{
	r->eg.edges = edges;
	r->eg.seconds = sa_hip_last_edges_seconds();
	return edges != NULL;
}

static bool take_tree(struct run *r, sa_linkage *tree)
{
	r->lk.tree = tree;
	if (r->o.method) {
		r->lk.seconds = sa_hip_last_agglomerate_seconds();
		r->lk.rescans = (long long)sa_hip_last_agglomerate_rescans();
	} else {
		r->lk.seconds = sa_hip_last_linkage_seconds();
		r->lk.rounds = sa_hip_last_linkage_rounds();
	}
	return tree != NULL;
}

static double last_quantity_seconds(struct quantity q)
{
	return q.norm ? sa_hip_last_normalize_seconds() : sa_hip_last_identity_seconds();
}

static void quantiles_answered(struct run *r)
{
	r->qt.done = true;
	r->qt.seconds = sa_hip_last_select_seconds();
	if (r->o.min_q >= 0)
		r->o.min_score = r->qt.values[r->o.min_q];
}

/* Which call answers the fractions when it takes one more alignment into device memory, decided here for every caller: with the score
 * graph where its cut is the only fraction (one alignment serves both), else with the tree where `with_tree` allows it and one is
 * still due, else a plain select in a pass of its own.  Makes that call; Q_FAILED with the message printed. */
enum q_call { Q_FAILED, Q_EDGES_AT_RANK, Q_LINKAGE_WITH_RANKS, Q_SELECT };
static enum q_call answer_quantiles(struct run *r, bool with_tree)
{
	const struct options *o = &r->o;
	enum q_call call;
	bool got;
	if (o->min_q >= 0 && o->nquant == 1 && !r->eg.edges) {
		call = Q_EDGES_AT_RANK;
		got = take_edges(r, sel_edges_at_rank(r->store.in, &r->sc, r->qt.ranks[0], &r->qt.values[0], &r->qt.below[0], r->q));
	} else if (with_tree && o->linkage && !r->lk.tree) {
		call = Q_LINKAGE_WITH_RANKS;
		got = take_tree(r, sel_linkage_with_ranks(r->store.in, &r->sc, o->method, r->qt.ranks, o->nquant, r->qt.values, r->qt.below, r->q));
	} else {
		call = Q_SELECT;
		got = sel_select(r->store.in, &r->sc, r->qt.ranks, o->nquant, r->qt.values, r->qt.below, r->q);
	}
	if (!got) {
		err("%s", sa_last_error());
		return Q_FAILED;
	}
	quantiles_answered(r);
	return call;
}

/* the first option given that a search (--query) does not go together with, or NULL: the --*-only modes, every selection from the
 * all-vs-all matrix, and -z (a search has no chunked dataset) */
static const char *query_conflict(const struct options *o)
{
	return o->neighbors_only ? "--neighbors-only" : o->edges_only ? "--edges-only" : o->linkage_only ? "--linkage-only"
	     : o->min_q >= 0 ? "--min-quantile" : o->has_min_score ? "--min-score" : o->clusters_q >= 0 ? "--clusters-quantile"
	     : o->has_clusters ? "--clusters" : o->has_method ? "--linkage-method" : o->linkage ? "--linkage" : o->nquant ? "--quantiles"
	     : o->normalize ? "--normalize" : o->identity ? "--identity" : o->compression ? "-z, --compression" : NULL;
}

/* is the matrix of -m one of the nucleotide tables?  (sa_matrix_load has accepted the name: it compares without case) */
static bool matrix_is_nucleotide(const char *name)
{
	for (int k = 0; k < sa_matrix_count(); k++)
		if (!strcasecmp(name, sa_matrix_name(k)))
			return sa_matrix_is_nucleotide(k) != 0;
	return false;
}

/* ---- the phases of main, in its order ------------------------------------------------------------------------------------------ */
/* options, -l, validation in the reference's terms (src/bio/align.c:130-201, ga.c:70-88, output.c:126-148) and the scoring.
 * returns 0 ok, 1 error, 2 handled-and-exit-success */
static int set_up(int argc, char **argv, struct run *r)
{
	struct options *o = &r->o;
	struct sa_scoring *sc = &r->sc;
	const int prc = parse_args(argc, argv, o);
	if (prc == 2)
		return 2;
	bool ok = prc == 0;
	if (ok && o->list) { /* -l: src/bio/matrices.c:27-33 */
		printf("\nListing available substitution matrices\n");
		for (int fam = 0; fam < 2; fam++) {
			printf("\n%s Matrices:\n  ", fam ? "Nucleotide" : "Amino");
			for (int k = 0, col = 0; k < sa_matrix_count(); k++)
				if (sa_matrix_is_nucleotide(k) == fam)
					printf("%-10s%s", sa_matrix_name(k), ++col % 5 ? "" : "\n  ");
			putchar('\n');
		}
		return 2;
	}
	if (ok && !o->input)
		ok = (err("Missing required option: -i, --input"), false);
	if (ok && !o->matrix)
		ok = (err("Missing required option: -m, --matrix"), false);
	if (ok && !o->align)
		ok = (err("Missing required option: -a, --align"), false);
	if (ok && o->output && o->no_write)
		ok = (err("Options -o, --output and -W, --no-write conflict"), false);
	if (ok && !o->output && !o->no_write)
		ok = (err("Missing required option: -o, --output"), false);
	if (ok && o->query_scores && !o->query)
		ok = (err("Option --query-scores requires --query"), false);
	if (ok && o->hits_by && !o->query)
		ok = (err("Option --hits-by requires --query: it ranks the hits of a search"), false);
	if (ok && o->has_hits_min && !o->query)
		ok = (err("Option --hits-min requires --query: it is the threshold of the hits of a search"), false);
	if (ok && o->has_hits_min && o->neighbors)
		ok = (err("Options --hits-min and -k, --neighbors conflict: a search writes the K best hits of every query or every hit at or "
			  "above T, not both"), false);
	if (ok && o->strands_both && !o->query)
		ok = (err("Option --strands both requires --query: it searches every query on both strands"), false);
	if (ok && o->fit && !o->query)
		ok = (err("Option --fit requires --query: it fits the queries of a search inside the database sequences"), false);
	if (ok && o->fit && o->has_hits_min)
		ok = (err("Options --fit and --hits-min conflict: the fitted search writes the K best hits of every query (-k)"), false);
	if (ok && o->fit && o->strands_both)
		ok = (err("Options --fit and --strands both conflict: the fitted search runs on the queries as written"), false);
	if (ok && o->fit && o->hits_by && o->hits_kind == 1)
		ok = (err("Options --fit and --hits-by %s conflict: the fitted hits are ranked by score or by one of identity-columns, identity-shorter, "
			  "identity-longer, identity-mean", o->hits_name), false);
	if (ok && o->query && !o->neighbors && !o->has_hits_min)
		ok = (err("Option --query requires -k, --neighbors (the number of hits per query) or --hits-min (the threshold of the hits)"), false);
	if (ok && o->query && query_conflict(o))
		ok = (err("Options --query and %s conflict: a search writes the hits of the queries and nothing selected from an all-vs-all matrix, "
			  "which it never computes", query_conflict(o)), false);
	if (ok && o->neighbors_only && !o->neighbors)
		ok = (err("Option --neighbors-only requires -k, --neighbors"), false);
	if (ok && o->alignments && !o->neighbors && !(o->query && o->has_hits_min))
		ok = (err("Option --alignments requires -k, --neighbors"), false);
	if (ok && o->has_min_score && o->min_q >= 0)
		ok = (err("Options --min-score and --min-quantile conflict: one threshold for the score graph"), false);
	if (ok && o->has_clusters && o->clusters_q >= 0)
		ok = (err("Options --clusters and --clusters-quantile conflict: one threshold for the clusters"), false);
	if (ok && o->min_q >= 0)
		o->has_min_score = true; /* (min_score itself follows from the selection) */
	if (ok && o->clusters_q >= 0)
		o->has_clusters = true;
	if (ok && o->edges_only && !o->has_min_score)
		ok = (err("Option --edges-only requires --min-score or --min-quantile"), false);
	if (ok && o->edges_only && o->neighbors)
		ok = (err("Options --edges-only and -k, --neighbors conflict: the neighbors need a pass of their own (use --min-score without --edges-only)"), false);
	if (ok && o->linkage_only && o->neighbors)
		ok = (err("Options --linkage-only and -k, --neighbors conflict: the neighbors need a pass of their own (use --linkage without --linkage-only)"), false);
	if (ok && o->linkage_only && o->has_min_score)
		ok = (err("Options --linkage-only and --min-score conflict: the score graph needs a pass of its own (use --linkage without --linkage-only)"), false);
	if (ok && o->has_method && !o->linkage)
		ok = (err("Option --linkage-method requires a tree: --linkage, --clusters, --clusters-quantile or --linkage-only"), false);
	if (ok && o->normalize && !o->neighbors && !o->has_min_score && !o->linkage && !o->nquant)
		ok = (err("Option --normalize requires something selected from the scores: -k, --min-score, --min-quantile, --linkage, --clusters, "
			  "--clusters-quantile or --quantiles (the similarity matrix itself stays raw)"), false);
	if (ok && o->identity && o->normalize)
		ok = (err("Options --identity and --normalize conflict: one quantity to select from"), false);
	if (ok && o->identity && !o->neighbors && !o->has_min_score && !o->linkage && !o->nquant)
		ok = (err("Option --identity requires something selected from the scores: -k, --min-score, --min-quantile, --linkage, --clusters, "
			  "--clusters-quantile or --quantiles (the similarity matrix itself stays raw)"), false);
	if (ok && sa_matrix_load(o->matrix, sc->lut, sc->sub))
		ok = (err("Invalid substitution matrix name"), false);
	if (ok && o->strands_both && !matrix_is_nucleotide(o->matrix))
		ok = (err("Options --strands both and -m %s conflict: only a nucleotide sequence has a reverse complement, and %s is an amino-acid "
			  "matrix", o->matrix, o->matrix), false);
	if (ok && (sc->method = sa_method_parse(o->align)) < 0)
		ok = (err("Invalid alignment method"), false);
	if (ok && o->fit && sc->method == SA_METHOD_SW)
		ok = (err("Options --fit and -a %s conflict: Smith-Waterman is local already; fit the queries with nw or ga", o->align), false);
	if (ok && o->gap_pen >= 0 && (o->gap_open >= 0 || o->gap_ext >= 0))
		ok = (err("Options -p and -s/-e conflict"), false);
	if (ok && sa_method_gap_kind(sc->method) == SA_GAP_LINEAR) {
		if (o->gap_open >= 0 || o->gap_ext >= 0)
			ok = (err("Affine gaps cannot be set for non-affine methods"), false);
		else if (o->gap_pen < 0)
			ok = (err("Missing required option: -p, --gap-penalty"), false);
	} else if (ok) {
		if (o->gap_pen >= 0)
			ok = (err("Gap penalty cannot be set for non-linear methods"), false);
		else if (o->gap_open < 0 || o->gap_ext < 0)
			ok = (err("Missing required option: -s, --gap-open and -e, --gap-extend"), false);
	}
	if (ok) {
		sc->gap_pen = o->gap_pen >= 0 ? -(int32_t)o->gap_pen : 0;
		sc->gap_opn = o->gap_open >= 0 ? -(int32_t)o->gap_open : 0;
		sc->gap_ext = o->gap_ext >= 0 ? -(int32_t)o->gap_ext : 0;
		if (sc->method == SA_METHOD_GA && sc->gap_opn == sc->gap_ext &&
		    ask("Equal affine gaps found, switch to Needleman-Wunsch?", true)) {
			sc->method = SA_METHOD_NW;
			sc->gap_pen = sc->gap_opn;
			sc->gap_opn = sc->gap_ext = SA_SCORE_MIN;
		}
	}
	if (ok && o->no_device)
		ok = (err("-C/--no-cuda: this build has no CPU alignment path (HIP device required)"), false);
	if (ok && o->output && access(o->output, F_OK) == 0) {
		if (!ask("Output file already exists. Do you want to DELETE it?", false))
			ok = (err("Output file exists and will not be overwritten"), false);
		else if (remove(o->output) != 0)
			ok = (err("Failed to delete existing output file"), false);
	}
	if (!ok) {
		fprintf(stderr, "Use %s -h, --help for usage information\n", r->argv0);
		return 1;
	}
	/* -T: host threads (validate_threads, src/system/os.c:466-473).  The alignment itself runs on the device; the
	 * host's parallel loops are the triangular->full expansion of the HDF5 writer and the CPU filter */
	if (o->threads > 0)
		omp_set_num_threads(o->threads);
	return 0;
}

static void banner(const struct run *r)
{
	const struct options *o = &r->o;
	info("SEQUENCE ALIGNER (MI355X / HIP)");
	info("Input: %s", o->input);
	if (o->output)
		info("Output: %s", o->output);
	info("Matrix: %s", o->matrix);
	info("Method: %s", sa_method_name(r->sc.method));
	if (r->sc.method == SA_METHOD_NW)
		info("Gap penalty: %d", r->sc.gap_pen);
	else
		info("Gap open: %d, extend: %d", r->sc.gap_opn, r->sc.gap_ext);
	if (o->filter > 0.0f)
		info("Filter threshold: %.1f%%", (double)o->filter * 100.0);
	if (o->query && o->has_hits_min) {
		if (o->hits_by && o->hits_kind)
			info("Queries: %s, every database sequence whose %s is at least %d parts per million (no similarity matrix)", o->query,
			     o->hits_name, o->hits_min);
		else
			info("Queries: %s, every database sequence that scores at least %d (no similarity matrix)", o->query, o->hits_min);
	} else if (o->query) {
		info("Queries: %s, the %d best database sequences of each (no similarity matrix)", o->query, o->neighbors);
		if (o->hits_by && o->hits_kind)
			info("Hits ranked by %s, in parts per million (the hit scores stay raw)", o->hits_name);
	} else if (o->neighbors)
		info("Neighbors: %d per sequence%s", o->neighbors, o->neighbors_only ? " (no similarity matrix)" : "");
	if (o->fit)
		info("Fit: every query whole, inside the database sequence (the database's overhang is free)");
	if (o->strands_both)
		info("Strands: both -- every query as written and reverse-complemented, folded on the device (the forward strand on a tie)");
	if (o->min_q >= 0)
		info("Score graph: pairs that score at least the %g quantile of the scores%s", o->quantiles[o->min_q],
		     o->edges_only ? " (no similarity matrix)" : "");
	else if (o->has_min_score)
		info("Score graph: pairs that score at least %d%s", o->min_score, o->edges_only ? " (no similarity matrix)" : "");
	if (o->linkage)
		info("%s tree%s", tree_name(o, true), o->linkage_only ? " (no similarity matrix)" : "");
	if (o->method && o->clusters_q >= 0)
		info("Clusters: the %s clusters merged at or above the %g quantile of the scores", tree_name(o, false), o->quantiles[o->clusters_q]);
	else if (o->method && o->has_clusters)
		info("Clusters: the %s clusters merged at or above %d", tree_name(o, false), o->clusters_at);
	else if (o->clusters_q >= 0)
		info("Clusters: connected components of the pairs that score at least the %g quantile of the scores", o->quantiles[o->clusters_q]);
	else if (o->has_clusters)
		info("Clusters: connected components of the pairs that score at least %d", o->clusters_at);
	if (o->nquant)
		info("Score quantiles: %d, selected on the device", o->nquant);
	if (o->normalize)
		info("Normalization: %s, in parts per million (the similarity matrix stays raw)", o->norm_name);
	if (o->identity)
		info("Percent identity over %s, in parts per million (the similarity matrix stays raw)", o->pid_name);
}

/* --query: the queries through the same reader and LUT as the input, never filtered; K against the database as filtered; room for the
 * hits.  The pairs of the run are the M x N of the rectangle */
static bool load_queries(struct run *r)
{
	const struct options *o = &r->o;
	const double t0 = now();
	if (sa_host_load(o->query, r->sc.lut, r->sc.gap_pen, o->dsv_column, o->dsv_has_header, &r->queries))
		return failed(sa_host_error());
	r->t_in += now() - t0;
	stamp("queries loaded");
	const size_t m = (size_t)r->queries.in.num;
	info("Loaded %d query sequences", r->queries.in.num);
	info("Average query length: %.2f", (double)r->queries.blob_bytes / (double)m - 1.0);
	if ((size_t)o->neighbors > r->n) {
		err("Hit count %d exceeds the %zu database sequences", o->neighbors, r->n);
		fprintf(stderr, "Use %s -h, --help for usage information\n", r->argv0);
		return false;
	}
	r->npairs = (long long)m * (long long)r->n * (o->strands_both ? 2 : 1);
	if (o->strands_both) { /* every query has a reverse complement the matrix takes, or the run ends here with the residue named */
		uint8_t *rc = malloc(r->queries.blob_bytes ? r->queries.blob_bytes : 1);
		if (!rc)
			return failed("Out of memory allocating search results");
		const bool can = sa_reverse_complement(r->queries.in, NULL, &r->sc, rc);
		free(rc);
		if (!can) {
			err("Options --strands both and --query %s conflict: %s", o->query, sa_last_error());
			fprintf(stderr, "Use %s -h, --help for usage information\n", r->argv0);
			return false;
		}
		if (!o->has_hits_min)
			r->st.hit = malloc(m * (size_t)o->neighbors);
		if (o->query_scores)
			r->st.rect = malloc(m * r->n);
		if ((!o->has_hits_min && !r->st.hit) || (o->query_scores && !r->st.rect))
			return failed("Out of memory allocating search results");
	}
	/* (--hits-min: the hits come back in arrays the library owns) */
	if (!o->has_hits_min) {
		r->sr.index = malloc(sizeof(int32_t) * m * (size_t)o->neighbors);
		r->sr.score = malloc(sizeof(int32_t) * m * (size_t)o->neighbors);
	}
	if (o->query_scores)
		r->sr.rect = malloc(sizeof(int32_t) * m * r->n);
	if ((!o->has_hits_min && (!r->sr.index || !r->sr.score)) || (o->query_scores && !r->sr.rect))
		return failed("Out of memory allocating search results");
	if (o->fit) {
		r->sr.db_begin = malloc(sizeof(int32_t) * m * (size_t)o->neighbors);
		r->sr.db_end = malloc(sizeof(int32_t) * m * (size_t)o->neighbors);
		if (!r->sr.db_begin || !r->sr.db_end)
			return failed("Out of memory allocating search results");
	}
	/* --hits-by: the quantity of the search, carried as the quantity of every selection is (kind 0: the scores, q stays empty) */
	if (o->hits_by && o->hits_kind) {
		r->norm_spec = (struct sa_norm){ o->hits_source, o->hits_rule, NULL };
		if (!o->has_hits_min)
			r->sr.value = malloc(sizeof(int32_t) * m * (size_t)o->neighbors);
		if (o->query_scores)
			r->sr.vrect = malloc(sizeof(int32_t) * m * r->n);
		if (o->hits_kind == 1) {
			r->norm_spec.denominators = malloc(sizeof(int32_t) * (r->n + m * (o->strands_both ? 2 : 1))); /* (both strands: N + 2 M) */
			r->q.norm = &r->norm_spec;
		} else
			r->q.pid = &o->hits_denom;
		if ((!o->has_hits_min && !r->sr.value) || (o->query_scores && !r->sr.vrect) || (r->q.norm && !r->norm_spec.denominators))
			return failed("Out of memory allocating search results");
	}
	return true;
}

/* the sequences, filtered, and what the selections need once their number is known: the ranks of the fractions, the quantity, room
 * for the neighbours */
static bool load_and_filter(struct run *r)
{
	struct options *o = &r->o;
	struct sa_host_store *store = &r->store;
	double t0 = now();
	if (sa_host_load(o->input, r->sc.lut, r->sc.gap_pen, o->dsv_column, o->dsv_has_header, store))
		return failed(sa_host_error());
	r->t_in = now() - t0;
	stamp("input loaded");
	t0 = now();
	const int32_t before = store->in.num;
	if (o->filter > 0.0f) { /* similarity relation on the device, greedy keep/drop in sequence order (filter.c:14-89) */
		uint8_t *keep = malloc((size_t)store->in.num);
		if (!keep || sa_hip_filter(store->in, o->filter, keep) < 0)
			return failed(keep ? sa_last_error() : "Out of memory during sequence filtering");
		if (sa_host_compact(store, keep) < 0)
			return failed(sa_host_error());
		free(keep);
	}
	r->t_filter = now() - t0;
	if (o->filter > 0.0f)
		info("Filtered out %d sequences", before - store->in.num);
	info("Loaded %d sequences", store->in.num);
	info("Average sequence length: %.2f", (double)store->blob_bytes / (double)store->in.num - 1.0);
	r->n = (size_t)store->in.num;
	r->npairs = (long long)r->n * ((long long)r->n - 1) / 2;
	if (o->query)
		return load_queries(r);

	if (o->neighbors && (long long)o->neighbors > (long long)store->in.num - 1) {
		err("Neighbor count %d exceeds the %d other sequences", o->neighbors, store->in.num - 1);
		fprintf(stderr, "Use %s -h, --help for usage information\n", r->argv0);
		return false;
	}
	for (int t = 0; t < o->nquant; t++) { /* the ranks of the fractions: P is known now */
		r->qt.ranks[t] = sa_score_rank((int64_t)r->npairs, o->quantiles[t]);
		if (r->qt.ranks[t] < 0)
			return failed("Score quantiles need at least two sequences");
	}
	/* --normalize: every selection goes the normalised way -- the tile job through sa_zjob_normalize, the rest through the *_norm
	 * calls; --identity: the same, through sa_zjob_identity and the *_pid calls */
	r->norm_spec = (struct sa_norm){ o->norm_source, o->norm_rule, NULL };
	if (o->normalize) {
		r->norm_spec.denominators = malloc(sizeof(int32_t) * r->n);
		if (!r->norm_spec.denominators)
			return failed("Out of memory allocating normalization denominators");
		r->q.norm = &r->norm_spec;
	}
	r->q.pid = o->identity ? &o->pid_denom : NULL;
	if (o->neighbors) {
		r->nb.index = malloc(sizeof(int32_t) * r->n * (size_t)o->neighbors);
		r->nb.score = malloc(sizeof(int32_t) * r->n * (size_t)o->neighbors);
		if (!r->nb.index || !r->nb.score)
			return failed("Out of memory allocating neighbor data");
	}
	return true;
}

/* Where the matrix goes.  output_load (src/io/output.c:35-55): a full matrix that exceeds 3/4 of the available RAM goes to temporary
 * file storage and is stored triangular; so is one the device(s) cannot hold */
static bool plan_output(struct run *r)
{
	const struct options *o = &r->o;
	const size_t n = r->n;
	r->out = (struct sa_output){ NULL, NULL, n, false };
	/* -z on a chunked dataset: the tiles are deflated on the device, from the packed scores where they were computed
	 * (include/seqalign_hip.h: sa_hip_tiles_begin / sa_zjob_next) -- no host matrix at all.  libhdf5's filter in the
	 * one writing thread (what flush_hdf5 leaves to H5Dwrite, src/io/format/hdf5.c:148-194) takes 41 CPU-minutes for config 5.
	 * SA_HOST_CPU_DEFLATE=1 keeps zlib at exactly the level asked for (all cores, sa_host_write_hdf5). */
	r->zchunk = sa_host_hdf5_chunk_dim(n);
	r->no_matrix = o->neighbors_only || o->edges_only || o->linkage_only || o->query != NULL; /* the matrix never leaves the device, or never is */
	r->device_deflate = !o->no_write && !r->no_matrix && n > 256 && !getenv("SA_HOST_MATRIX") &&
			    (o->compression > 0 ? !getenv("SA_HOST_CPU_DEFLATE") && !getenv("SA_HOST_SERIAL_DEFLATE")
						/* without -z the same walk returns the tiles as they are: H5Dwrite_chunk instead of H5Dwrite's
						 * gather of every tile out of N-wide rows.  On several devices the plain path stays with sa_hip_align
						 * (tiles dealt by DP work, RCCL all-gather: the whole matrix on every device and in host memory);
						 * with -z the walk itself runs on all of them (sa_hip_tiles_begin: block b -> device b mod n) */
						: sa_hip_device_count() == 1);
	if (r->device_deflate) {
		/* the packed scores + one tile row: raw, or raw + worst-case slots and streams (1 + 2 x 2.02 x the row's raw bytes); the
		 * pair parse (-z 7..9) keeps two more bytes per element: what its match finder leaves for the encoder */
		const size_t row_raw = ((n + r->zchunk - 1) / r->zchunk) * r->zchunk * r->zchunk * sizeof(int32_t);
		r->device_deflate = sa_hip_memory(sizeof(int32_t) * (size_t)r->npairs + (o->compression ? 6 : 1) * row_raw +
						  (o->compression >= SA_HIP_Z_PAIR_LEVEL ? row_raw / 2 : 0));
		stamp("device memory probed (runtime up)");
	}
	if (o->no_write || r->device_deflate || r->no_matrix)
		return true;
	const bool tmpf = sa_host_matrix_needs_file(n);
	r->out.triangular = tmpf || !sa_hip_memory(sizeof(int32_t) * n * n);
	stamp("device memory probed (runtime up)");
	info("Similarity Matrix dimensions: %zu x %zu%s", n, n, r->out.triangular ? " (stored triangular)" : "");
	if (tmpf)
		info("Similarity Matrix size exceeds memory limits, creating temporary file storage");
	const double t0 = now();
	r->out.matrix = sa_host_matrix_alloc(n, r->out.triangular, tmpf);
	if (!r->out.matrix)
		return failed(sa_host_error());
	stamp("matrix allocated");
	/* page-lock it for the device->host copies while it is being set up (a file-backed matrix is larger than
	 * RAM by definition and stays pageable: the library stages those copies) */
	if (!tmpf) {
		const size_t bytes = sizeof(int32_t) * (r->out.triangular ? n * (n - 1) / 2 : n * n);
		/* (the library's own rule, sa_ctx_align_host: never lock more than half of what is available -- a
		 * registration of 70 % of free RAM thrashes or meets the OOM killer instead of failing cleanly) */
		const size_t avail = sa_host_available_memory();
		r->pinned = bytes && (!avail || bytes <= avail / 2) && sa_hip_host_register(r->out.matrix, bytes) == 0;
	}
	r->t_out += now() - t0;
	stamp("matrix page-locked");
	return true;
}

/* what a finished tile job answered from its matrix, and what it left to the second passes, under -V */
static void job_says(bool got, const char *what, const char *how)
{
	if (got)
		verb("%s %s from the device's finished matrix (no second alignment)", what, how);
	else
		verb("%s: %s", what, sa_last_error());
}

/* The tile job: the alignment runs on the device while the finished tiles are written: the tiles whose larger tile index is b
 * need exactly column block b (include/seqalign_hip.h: sa_hip_tiles_begin).  The reference's phases (src/main.c:31-34,
 * bench_align / bench_io) overlap here: "Alignment" is the device's alignment time, "Output" the rest of the wall time of
 * this section.  The finished matrix is still on the device afterwards: what the job can answer from it is not aligned twice, what
 * it cannot (a message under -V) is left to the second passes. */
static bool run_tile_job(struct run *r)
{
	struct options *o = &r->o;
	info("Similarity Matrix dimensions: %zu x %zu (%s on the device, tile by tile)", r->n, r->n, o->compression ? "deflated" : "tiled");
	double t0 = now();
	sa_zjob *job = sa_hip_tiles_begin(r->store.in, &r->sc, r->zchunk, (int)o->compression);
	if (!job)
		return failed(sa_last_error());
	r->t_setup = now() - t0;
	stamp("sa_hip_tiles_begin returned");
	t0 = now();
	struct tile_feed feed = { job, sa_zjob_tiles_per_row(job), r->show_progress };
	if (sa_host_write_hdf5_streams(o->output, &r->store, o->compression, next_tiles, &feed)) {
		err("%s (%s)", sa_host_error(), sa_last_error());
		return false;
	}
	finish_progress(r);
	r->t_align = sa_zjob_align_seconds(job);
	const double section = now() - t0;
	r->t_out += section > r->t_align ? section - r->t_align : 0.0;
	double enc_ms = 0, copy_ms = 0;
	uint64_t raw = 0, outb = 0;
	sa_zjob_stats(job, &enc_ms, &copy_ms, &raw, &outb);
	verb("%s on the device: %.2f GB -> %.2f GB (%.2f : 1); the writer waited %.0f ms for the encoder, %.0f ms for gather + copy",
	     o->compression ? "Deflated" : "Tiled", (double)raw / 1e9, (double)outb / 1e9, outb ? (double)raw / (double)outb : 0.0, enc_ms,
	     copy_ms);
	/* --normalize / --identity: every tile is written, raw; the device's matrix is rewritten in place for what is selected from it.
	 * A job that cannot (the matrix dealt over several jobs) answers nothing below */
	bool job_answers = true;
	if (r->q.norm || r->q.pid) {
		job_answers = (r->q.norm ? sa_zjob_normalize(job, r->q.norm) : sa_zjob_identity(job, *r->q.pid)) == 0;
		if (!job_answers)
			verb("%s: %s", r->q.norm ? "Normalization" : "Identity", sa_last_error());
		else
			verb("%s in place on the device (the tiles written are raw)", r->q.norm ? "Scores normalised" : "Percent identity");
		r->t_quantity = job_answers ? last_quantity_seconds(r->q) : 0;
	}
	if (o->neighbors && job_answers) {
		r->nb.done = sa_zjob_neighbors(job, o->neighbors, r->nb.index, r->nb.score) == 0;
		r->nb.seconds = sa_hip_last_neighbors_seconds();
		job_says(r->nb.done, "Neighbors", "selected");
	}
	if (o->nquant && job_answers) { /* first: the cut of what follows */
		const bool got = sa_zjob_select(job, r->qt.ranks, o->nquant, r->qt.values, r->qt.below) == 0;
		if (got)
			quantiles_answered(r);
		job_says(got, "Score quantiles", "selected");
	}
	if (o->has_min_score && (o->min_q < 0 || r->qt.done) && job_answers)
		job_says(take_edges(r, sa_zjob_edges(job, o->min_score)), "Score graph", "built");
	if (o->linkage && job_answers)
		job_says(take_tree(r, o->method ? sa_zjob_agglomerate(job, o->method) : sa_zjob_linkage(job)), tree_title(o), "built");
	sa_zjob_destroy(job);
	stamp("HDF5 written");
	return true;
}

/* --linkage-only, --edges-only, --neighbors-only: no host matrix, no tiles, no matrix transfer: align into device memory, select
 * there, copy back the selection (12 (N - 1) bytes, 8 N + 8 E bytes, 2 N K ints).  Set-up is the call less its two device times. */
static bool run_only(struct run *r)
{
	const struct options *o = &r->o;
	if (o->linkage_only)
		info("Similarity Matrix stays on the device: the %s tree is built there", tree_name(o, false));
	else if (o->edges_only && o->min_q >= 0)
		info("Similarity Matrix stays on the device: the cut and the pairs at or above it are selected there");
	else if (o->edges_only)
		info("Similarity Matrix stays on the device: the pairs that score at least %d are selected there", o->min_score);
	else
		info("Similarity Matrix stays on the device: %d neighbors per sequence are selected there", o->neighbors);
	const double t0 = now();
	bool got = true;
	if (o->neighbors_only) {
		got = r->nb.done = sel_neighbors(r->store.in, &r->sc, o->neighbors, r->nb.index, r->nb.score, r->q);
	} else if (o->nquant) { /* with the graph or the tree from one alignment where that serves; further fractions of a graph in a pass of their own */
		const enum q_call served = answer_quantiles(r, o->linkage_only);
		if (served == Q_FAILED)
			return false;
		r->qt.second_pass = served == Q_SELECT;
	}
	if (got && o->edges_only && !r->eg.edges)
		got = take_edges(r, sel_edges(r->store.in, &r->sc, o->min_score, r->q));
	if (got && o->linkage_only && !r->lk.tree)
		got = take_tree(r, sel_linkage(r->store.in, &r->sc, o->method, r->q));
	if (!got)
		return failed(sa_last_error());
	const double call = now() - t0;
	stamp(o->linkage_only ? o->method ? "sa_hip_agglomerate returned" : "sa_hip_linkage returned" : o->edges_only ? "sa_hip_edges returned" : "sa_hip_neighbors returned");
	finish_progress(r);
	r->t_align = sa_hip_last_align_seconds();
	const double t_sel = o->linkage_only ? r->lk.seconds : o->edges_only ? r->eg.seconds : (r->nb.seconds = sa_hip_last_neighbors_seconds());
	r->t_setup = call > r->t_align + t_sel ? call - r->t_align - t_sel : 0.0;
	return true;
}

/* --query: the M x N rectangle and the hits of every query in one call, in batches of queries sized by the library; only the hits
 * (and with --query-scores the rectangle) come back.  Set-up is the call less its device time. */
static bool run_search(struct run *r)
{
	const struct options *o = &r->o;
	if (o->has_hits_min)
		info("Search: %d queries against %zu database sequences, the hits at or above %d selected on the device", r->queries.in.num, r->n,
		     o->hits_min);
	else
		info("Search: %d queries against %zu database sequences, %d hits per query selected on the device", r->queries.in.num, r->n, o->neighbors);
	const double t0 = now();
	/* the one call that fits (the *_norm call with norm == NULL is sa_hip_search itself) */
	if (o->has_hits_min) {
		r->ab.list = o->strands_both ? sa_hip_search_above_strands(r->store.in, r->queries.in, &r->sc, NULL, o->hits_min, r->q.norm, r->q.pid)
					     : sa_hip_search_above(r->store.in, r->queries.in, &r->sc, o->hits_min, r->q.norm, r->q.pid);
		if (!r->ab.list)
			return failed(sa_last_error());
		int64_t count = 0;
		(void)sa_hitlist_index(r->ab.list, &count);
		r->ab.count = (long long)count;
	} else if (o->fit) {
		if (!sa_hip_search_fit(r->store.in, r->queries.in, &r->sc, o->neighbors, r->q.pid ? *r->q.pid : -1, r->sr.index, r->sr.value, r->sr.score,
				       r->sr.db_begin, r->sr.db_end, r->sr.rect, r->sr.vrect))
			return failed(sa_last_error());
	} else if (o->strands_both) {
		if (!sa_hip_search_strands(r->store.in, r->queries.in, &r->sc, NULL, o->neighbors, r->sr.index, r->sr.value, r->sr.score, r->st.hit,
					   r->sr.rect, r->sr.vrect, r->st.rect, r->q.norm, r->q.pid))
			return failed(sa_last_error());
	} else if (!(r->q.pid ? sa_hip_search_pid(r->store.in, r->queries.in, &r->sc, o->neighbors, r->sr.index, r->sr.value, r->sr.score, r->sr.rect,
					   r->sr.vrect, *r->q.pid)
		       : sa_hip_search_norm(r->store.in, r->queries.in, &r->sc, o->neighbors, r->sr.index, r->sr.value, r->sr.score, r->sr.rect,
					    r->sr.vrect, r->q.norm)))
		return failed(sa_last_error());
	const double call = now() - t0;
	stamp("sa_hip_search returned");
	r->t_quantity = o->fit ? 0.0 : sa_hip_last_search_quantity_seconds(); /* (--fit: the one sweep delivers score and identity) */
	r->st.seconds = o->strands_both ? sa_hip_last_search_strands_seconds() : 0.0;
	finish_progress(r);
	sa_hip_last_search_breakdown(&r->t_align, &r->sr.gather_seconds, &r->sr.hits_seconds, &r->sr.batches);
	const double device = sa_hip_last_search_seconds() + (r->q.norm ? r->t_quantity : 0.0) + r->st.seconds;
	r->t_setup = call > device ? call - device : 0.0;
	if (o->has_hits_min && o->query_scores) {
		/* the rectangles do not come back with the hit list: a second alignment, index NULL, delivers them */
		const double t1 = now();
		if (!(o->strands_both ? sa_hip_search_strands(r->store.in, r->queries.in, &r->sc, NULL, 0, NULL, NULL, NULL, NULL, r->sr.rect, r->sr.vrect,
							      r->st.rect, r->q.norm, r->q.pid)
		      : r->q.pid    ? sa_hip_search_pid(r->store.in, r->queries.in, &r->sc, 0, NULL, NULL, NULL, r->sr.rect, r->sr.vrect, *r->q.pid)
				    : sa_hip_search_norm(r->store.in, r->queries.in, &r->sc, 0, NULL, NULL, NULL, r->sr.rect, r->sr.vrect, r->q.norm)))
			return failed(sa_last_error());
		r->ab.rect_seconds = now() - t1;
		stamp("sa_hip_search (rectangles) returned");
	}
	return true;
}

/* --query --alignments: the M x K pairs (query q, hit_indices[q][t]), row-major, traced back on a search context: a = N + q of the
 * concatenated store, b = the hit, so every record comes back with the query as a (include/seqalign_hip.h: search) */
static bool trace_hits(struct run *r)
{
	const struct options *o = &r->o;
	if (!o->alignments)
		return true;
	const int64_t *offsets = o->has_hits_min ? sa_hitlist_offsets(r->ab.list, NULL) : NULL;
	const int32_t *index = o->has_hits_min ? sa_hitlist_index(r->ab.list, NULL) : r->sr.index;
	const size_t np = o->has_hits_min ? (size_t)r->ab.count : (size_t)r->queries.in.num * (size_t)o->neighbors;
	if (np == 0) /* (--hits-min above every value: no pair to trace, the datasets are written with extent 0) */
		return true;
	int32_t *pa = malloc(sizeof(int32_t) * np);
	if (!pa)
		return failed("Out of memory allocating alignment pairs");
	/* --strands both: a reverse hit is traced on the row of the query's reverse complement, M rows on (include/seqalign_hip.h) */
	const uint8_t *strand = !o->strands_both ? NULL : o->has_hits_min ? sa_hitlist_strand(r->ab.list) : r->st.hit;
	const int32_t m = r->queries.in.num;
	if (o->has_hits_min) { /* the E pairs (query q, its hits) in the order of the hit list */
		for (int32_t q = 0; q < r->queries.in.num; q++)
			for (int64_t t = offsets[q]; t < offsets[q + 1]; t++)
				pa[t] = (int32_t)r->n + q + (strand && strand[t] ? m : 0);
	} else
		for (size_t t = 0; t < np; t++) /* (--fit: sa_ctx_fit_alignments takes the query itself, not its place in the store) */
			pa[t] = (int32_t)((o->fit ? 0 : r->n) + t / (size_t)o->neighbors) + (strand && strand[t] ? m : 0);
	sa_ctx *ctx = o->strands_both ? sa_ctx_create_search_strands(0, r->store.in, r->queries.in, &r->sc, NULL)
				      : sa_ctx_create_search(0, r->store.in, r->queries.in, &r->sc);
	r->sr.alns = !ctx ? NULL : o->fit ? sa_ctx_fit_alignments(ctx, pa, index, (int64_t)np) : sa_ctx_alignments(ctx, pa, index, (int64_t)np);
	free(pa);
	if (ctx)
		sa_ctx_destroy(ctx);
	if (!r->sr.alns)
		return failed(sa_last_error());
	r->trace.seconds = sa_hip_last_alignments_seconds();
	stamp("sa_ctx_alignments returned");
	return true;
}

static bool write_search_plain(struct run *r, const uint32_t *cigar, int64_t runs);

/* --query: everything of a search into one file of its own */
static bool write_search(struct run *r)
{
	const struct options *o = &r->o;
	int64_t runs = 0;
	const uint32_t *cigar = r->sr.alns ? sa_alns_cigar(r->sr.alns, &runs) : NULL;
	r->trace.runs = (long long)runs;
	if (o->strands_both) /* the files of a search, then the strands added to them */
		return write_search_plain(r, cigar, runs) &&
		       WRITE_OUT(r, sa_host_write_search_strands(o->output, &r->store, &r->queries, o->has_hits_min ? 0 : o->neighbors, r->st.hit,
								 o->has_hits_min ? (int64_t)r->ab.count : -1, o->has_hits_min ? sa_hitlist_strand(r->ab.list) : NULL,
								 r->st.rect, r->q.norm ? r->q.norm->denominators + r->n + r->queries.in.num : NULL),
				 "strands written");
	if (o->fit) /* the file of a search, then where the queries sit */
		return write_search_plain(r, cigar, runs) &&
		       WRITE_OUT(r, sa_host_write_search_fit(o->output, &r->store, &r->queries, o->neighbors, r->sr.index, r->sr.db_begin, r->sr.db_end),
				 "fit spans written");
	return write_search_plain(r, cigar, runs);
}

static bool write_search_plain(struct run *r, const uint32_t *cigar, int64_t runs)
{
	const struct options *o = &r->o;
	if (o->has_hits_min)
		return WRITE_OUT(r, sa_host_write_search_list(o->output, &r->store, &r->queries, sa_hitlist_offsets(r->ab.list, NULL),
							      sa_hitlist_index(r->ab.list, NULL), sa_hitlist_score(r->ab.list), o->hits_min,
							      sa_hitlist_value(r->ab.list), r->q.norm ? 1 : r->q.pid ? 2 : 0, r->q.norm ? r->q.norm->source : 0,
							      r->q.norm ? r->q.norm->rule : r->q.pid ? *r->q.pid : 0, r->q.norm ? r->q.norm->denominators : NULL,
							      r->sr.rect, r->sr.vrect, o->alignments, r->sr.alns ? sa_alns_records(r->sr.alns) : NULL, cigar,
							      runs), "hit list written");
	if (!WRITE_OUT(r, sa_host_write_search(o->output, &r->store, &r->queries, o->neighbors, r->sr.index, r->sr.score, r->sr.rect,
					       r->sr.alns ? sa_alns_records(r->sr.alns) : NULL, cigar, runs), "search written"))
		return false;
	if (!r->q.norm && !r->q.pid)
		return true;
	return WRITE_OUT(r, sa_host_write_search_values(o->output, &r->store, &r->queries, o->neighbors, r->sr.value, r->q.norm ? 1 : 2,
							r->q.norm ? r->q.norm->source : 0, r->q.norm ? r->q.norm->rule : *r->q.pid,
							r->q.norm ? r->q.norm->denominators : NULL, r->sr.vrect), "hit values written");
}

/* the matrix into host memory, then the file from there */
static bool run_host_matrix(struct run *r)
{
	const double t0 = now();
	if (!sa_hip_align(r->store.in, r->out, &r->sc))
		return failed(sa_last_error());
	r->t_align = now() - t0;
	stamp("sa_hip_align returned");
	finish_progress(r);
	/* the reference times the launch/copy loop only (bench_align_start..end inside cuda_align,
	 * src/interface/seqalign_cuda.c:182,292): device set-up and uploads are not part of "Alignment" */
	r->t_setup = r->t_align - sa_hip_last_align_seconds();
	r->t_align = sa_hip_last_align_seconds();
	r->schedule = sa_hip_last_align_path();
	return WRITE_OUT(r, sa_host_write_hdf5(r->o.output, &r->store, r->out.matrix, r->out.triangular, r->o.compression), "HDF5 written");
}

/* ---- the second passes: what the first pass left unanswered.  Its paths other than a tile job on one device (N <= 256, SA_HOST_*
 * switches, -W, several devices, a walk dealt over several jobs) no longer hold the matrix on one device: a second pass aligns into
 * device memory again and selects there ---- */
#define SECOND_PASS "%s: a second alignment pass into device memory (the matrix of the first is not on one device any more)"

static bool passed(bool got, bool *second_pass, const char *what)
{
	if (!got)
		return failed(sa_last_error());
	*second_pass = true;
	stamp(what);
	return true;
}

static bool pass_neighbors(struct run *r)
{
	if (!r->o.neighbors || r->nb.done)
		return true;
	verb(SECOND_PASS, "Neighbors");
	r->nb.done = sel_neighbors(r->store.in, &r->sc, r->o.neighbors, r->nb.index, r->nb.score, r->q);
	r->nb.seconds = sa_hip_last_neighbors_seconds();
	return passed(r->nb.done, &r->nb.second_pass, "sa_hip_neighbors returned");
}

/* the fractions -- with what the cut feeds where one alignment can serve both, by itself otherwise -- and what they make of the cuts */
static bool pass_quantiles(struct run *r)
{
	struct options *o = &r->o;
	if (o->nquant && !r->qt.done) {
		verb(SECOND_PASS, "Score quantiles");
		const enum q_call call = answer_quantiles(r, true);
		if (call == Q_FAILED)
			return false;
		r->qt.second_pass = true;
		r->eg.second_pass = call == Q_EDGES_AT_RANK;
		r->lk.second_pass = call == Q_LINKAGE_WITH_RANKS;
		stamp("score quantiles returned");
	}
	if (!r->qt.done)
		return true;
	if (o->min_q >= 0) {
		o->min_score = r->qt.values[o->min_q];
		info("Score graph: T = %d, the score at rank %lld of %lld: %lld pairs score at least T", o->min_score, (long long)r->qt.ranks[o->min_q],
		     r->npairs, r->npairs - (long long)r->qt.below[o->min_q]);
	}
	if (o->clusters_q >= 0) {
		o->clusters_at = r->qt.values[o->clusters_q];
		info("Clusters: T = %d, the score at rank %lld of %lld: %lld pairs score at least T", o->clusters_at,
		     (long long)r->qt.ranks[o->clusters_q], r->npairs, r->npairs - (long long)r->qt.below[o->clusters_q]);
	}
	return true;
}

static bool pass_edges(struct run *r)
{
	if (!r->o.has_min_score || r->eg.edges)
		return true;
	verb(SECOND_PASS, "Score graph");
	return passed(take_edges(r, sel_edges(r->store.in, &r->sc, r->o.min_score, r->q)), &r->eg.second_pass, "sa_hip_edges returned");
}

static bool pass_linkage(struct run *r)
{
	if (!r->o.linkage || r->lk.tree)
		return true;
	verb(SECOND_PASS, tree_title(&r->o));
	return passed(take_tree(r, sel_linkage(r->store.in, &r->sc, r->o.method, r->q)), &r->lk.second_pass,
		      r->o.method ? "sa_hip_agglomerate returned" : "sa_hip_linkage returned");
}

/* ---- writing the selections: each into the file the matrix made, or into one of its own when there is no matrix ---- */
static bool write_neighbors(struct run *r)
{
	return !r->o.neighbors || WRITE_OUT(r, sa_host_write_neighbors(r->o.output, &r->store, r->o.neighbors, r->nb.index, r->nb.score,
									 r->o.neighbors_only ? 1 : 0), "neighbors written");
}

/* --alignments: the N x K pairs (r, neighbor_indices[r][t]), row-major: traced back on the device (include/seqalign_hip.h), written */
static bool trace_alignments(struct run *r)
{
	const struct options *o = &r->o;
	if (!o->alignments)
		return true;
	const size_t np = r->n * (size_t)o->neighbors;
	int32_t *pa = malloc(sizeof(int32_t) * np);
	if (!pa)
		return failed("Out of memory allocating alignment pairs");
	for (size_t t = 0; t < np; t++)
		pa[t] = (int32_t)(t / (size_t)o->neighbors);
	sa_alns *alns = sa_hip_alignments(r->store.in, &r->sc, pa, r->nb.index, (int64_t)np);
	free(pa);
	if (!alns)
		return failed(sa_last_error());
	r->trace.seconds = sa_hip_last_alignments_seconds(); /* (reported by itself: the Alignment phase stays the all-vs-all scores) */
	stamp("sa_hip_alignments returned");
	int64_t runs = 0;
	const uint32_t *cigar = sa_alns_cigar(alns, &runs);
	r->trace.runs = (long long)runs;
	if (!WRITE_OUT(r, sa_host_write_alignments(o->output, &r->store, o->neighbors, sa_alns_records(alns), cigar, runs), "alignments written"))
		return false;
	sa_alns_destroy(alns);
	return true;
}

static bool write_edges(struct run *r)
{
	if (!r->eg.edges)
		return true;
	int64_t count = 0;
	const int32_t *index = sa_edges_index(r->eg.edges, &count);
	r->eg.count = (long long)count;
	if (!WRITE_OUT(r, sa_host_write_edges(r->o.output, &r->store, sa_edges_offsets(r->eg.edges, NULL), index, sa_edges_score(r->eg.edges),
					      r->o.edges_only ? 1 : 0), "edges written"))
		return false;
	sa_edges_destroy(r->eg.edges);
	return true;
}

/* the tree, and with --clusters the labels it gives at the cut */
static bool write_linkage(struct run *r)
{
	const struct options *o = &r->o;
	if (!r->lk.tree)
		return true;
	const int32_t *pairs = sa_linkage_pairs(r->lk.tree, &r->lk.merges), *score = sa_linkage_score(r->lk.tree);
	int32_t *labels = NULL;
	if (o->has_clusters) {
		labels = malloc(sizeof(int32_t) * r->n);
		if (!labels)
			return failed("Out of memory allocating cluster labels");
		r->lk.clusters = (o->method ? sa_agglo_labels : sa_linkage_labels)(pairs, score, r->store.in.num, o->clusters_at, labels);
		if (r->lk.clusters < 0)
			return failed(sa_last_error());
		verb("Clusters: %d at score >= %d", r->lk.clusters, o->clusters_at);
	}
	if (!WRITE_OUT(r, sa_host_write_linkage(o->output, &r->store, pairs, score, labels, o->linkage_only ? 1 : 0), "linkage written"))
		return false;
	if (o->has_method && !WRITE_OUT(r, sa_host_write_linkage_method(o->output, o->method), "linkage method written"))
		return false;
	free(labels);
	sa_linkage_destroy(r->lk.tree);
	return true;
}

/* last: whatever was asked for beside them has made the file by now.  The quantiles, then what says which quantity all of it was
 * selected from: the denominators came back with whichever call normalised */
static bool write_quantiles_and_quantity(struct run *r)
{
	const struct options *o = &r->o;
	if (r->qt.done && !WRITE_OUT(r, sa_host_write_quantiles(o->output, &r->store, o->quantiles, r->qt.values, r->qt.below, o->nquant,
								 o->min_q >= 0 ? &o->min_score : NULL, o->clusters_q >= 0 ? &o->clusters_at : NULL, 0),
				     "quantiles written"))
		return false;
	if (r->q.norm && !WRITE_OUT(r, sa_host_write_normalization(o->output, &r->store, r->norm_spec.denominators, r->norm_spec.source,
								    r->norm_spec.rule), "normalization written"))
		return false;
	if (r->q.pid && !WRITE_OUT(r, sa_host_write_identity(o->output, *r->q.pid), "identity rule written"))
		return false;
	if ((r->q.pid || r->q.norm) && r->t_quantity == 0)
		r->t_quantity = last_quantity_seconds(r->q); /* (the *_pid / *_norm calls: the last of them) */
	return true;
}

/* -B: src/util/benchmark.c:50-64 */
static void report(const struct run *r)
{
	const struct options *o = &r->o;
	static const char AGAIN[] = ", after a second alignment pass into device memory";
	printf("Timing breakdown:\n  Input: %.3f sec\n  Filter: %.3f sec\n  Alignment: %.3f sec\n  Output: %.3f sec\n"
	       "  Total: %.3f sec\n",
	       r->t_in, r->t_filter, r->t_align, r->t_out, r->t_in + r->t_filter + r->t_align + r->t_out);
	printf("  (device set-up and upload, outside the phases as in the reference: %.3f sec)\n", r->t_setup);
	printf("  (schedule: %s)\n", r->device_deflate ? (o->compression ? "column blocks into device memory, their tiles deflated on the device and written meanwhile"
									  : "column blocks into device memory, their tiles delivered as HDF5 chunks meanwhile")
			       : o->query ? "only the query-database rectangle is aligned, in batches of queries; only the hits come back"
			       : o->linkage_only && o->method == SA_AGGLO_COMPLETE ? "the packed matrix stays in device memory, only the complete-linkage tree comes back"
			       : o->linkage_only && o->method == SA_AGGLO_AVERAGE ? "the packed matrix stays in device memory, only the average-linkage tree comes back"
			       : o->linkage_only ? "the packed matrix stays in device memory, only the single-linkage tree comes back"
			       : o->edges_only ? "the packed matrix stays in device memory, only the edges come back"
			       : o->neighbors_only ? "the packed matrix stays in device memory, only the neighbors come back"
			       : r->schedule == 2 ? "tiles dealt over the devices, RCCL all-gather of the dense shares, placement on every device"
						  : "every device delivers its slice of the packed index straight into the host matrix");
	if (o->query) {
		if (o->has_hits_min) {
			printf("  (hits at or above %d on the device: %lld hits, count + scan + fill %.6f sec; rows gathered in %.6f sec; %d batches of queries)\n",
			       o->hits_min, r->ab.count, r->sr.hits_seconds, r->sr.gather_seconds, r->sr.batches);
			if (o->query_scores)
				printf("  (--query-scores: a second alignment of the rectangle delivered it, %.3f sec, outside the phases)\n", r->ab.rect_seconds);
		} else
			printf("  (hit selection on the device, K = %d: %.6f sec; rows gathered in %.6f sec; %d batches of queries)\n", o->neighbors,
			       r->sr.hits_seconds, r->sr.gather_seconds, r->sr.batches);
		if (o->strands_both)
			printf("  (both strands searched: every query as written and reverse-complemented; fold + strands of the hits on the device: %.6f sec)\n",
			       r->st.seconds);
		if (r->q.norm)
			printf("  (hits by %s on the device: denominators + sweep over %lld pairs, %.6f sec)\n", o->hits_name, r->npairs, r->t_quantity);
		if (r->q.pid)
			printf("  (hits by %s on the device: one identity sweep over %lld pairs, scores and values together, %.6f sec)\n", o->hits_name,
			       r->npairs, r->t_quantity);
		if (o->alignments)
			printf("  (alignments of the %lld hit pairs on the device, fill + walk: %.6f sec, %lld CIGAR runs)\n",
			       o->has_hits_min ? r->ab.count : (long long)r->queries.in.num * o->neighbors, r->trace.seconds, r->trace.runs);
	} else if (o->neighbors)
		printf("  (neighbor selection on the device, K = %d: %.6f sec%s)\n", o->neighbors, r->nb.seconds, r->nb.second_pass ? AGAIN : "");
	if (o->alignments && !o->query)
		printf("  (alignments of the %lld neighbor pairs on the device, fill + walk: %.6f sec, %lld CIGAR runs)\n",
		       (long long)r->store.in.num * o->neighbors, r->trace.seconds, r->trace.runs);
	if (o->nquant)
		printf("  (Score quantiles on the device: %d ranks of %lld pairs, %.6f sec%s)\n", o->nquant, r->npairs, r->qt.seconds,
		       r->qt.second_pass ? AGAIN : "");
	if (o->has_min_score)
		printf("  (score graph on the device, min score = %d: %lld edges, %.6f sec%s)\n", o->min_score, r->eg.count, r->eg.seconds,
		       r->eg.second_pass ? AGAIN : "");
	if (o->linkage && o->method)
		printf("  (%s tree on the device: %d merges, %lld row rescans, %.6f sec%s)\n", tree_name(o, false), r->lk.merges, r->lk.rescans,
		       r->lk.seconds, r->lk.second_pass ? AGAIN : "");
	else if (o->linkage)
		printf("  (single-linkage tree on the device: %d merges, %d rounds, %.6f sec%s)\n", r->lk.merges, r->lk.rounds, r->lk.seconds,
		       r->lk.second_pass ? AGAIN : "");
	if (o->has_clusters)
		printf("  (clusters at score >= %d: %d)\n", o->clusters_at, r->lk.clusters);
	if (r->q.norm && !o->query)
		printf("  (Normalisation on the device, %s: denominators + sweep over %lld pairs, %.6f sec)\n", o->norm_name, r->npairs, r->t_quantity);
	if (r->q.pid && !o->query)
		printf("  (Percent identity on the device, over %s: one sweep over %lld pairs, %.6f sec)\n", o->pid_name, r->npairs, r->t_quantity);
	printf("Alignments per second: %.2f\n", r->t_align > 0 ? (double)r->npairs / r->t_align : 0.0);
}

static void release(struct run *r)
{
	if (r->pinned)
		sa_hip_host_unregister(r->out.matrix);
	sa_host_matrix_free(r->out.matrix, r->n, r->out.triangular);
	free(r->nb.index);
	free(r->nb.score);
	free(r->norm_spec.denominators);
	if (r->sr.alns)
		sa_alns_destroy(r->sr.alns);
	sa_hitlist_destroy(r->ab.list);
	free(r->sr.index);
	free(r->sr.score);
	free(r->sr.rect);
	free(r->sr.value);
	free(r->sr.vrect);
	free(r->sr.db_begin);
	free(r->sr.db_end);
	free(r->st.hit);
	free(r->st.rect);
	sa_host_store_free(&r->queries);
	sa_host_store_free(&r->store);
	stamp("released");
}

int main(int argc, char **argv)
{
	t_process0 = now();
	static struct run run;
	struct run *r = &run;
	r->argv0 = argv[0];
	const int rc = set_up(argc, argv, r);
	if (rc)
		return rc == 2 ? 0 : 1;
	banner(r);
	stamp("options parsed");
	if (!load_and_filter(r) || !plan_output(r))
		return 1;

	info("Performing %lld pairwise alignments", r->npairs);
	/* progress (ppercent / pproportc in the reference's launch loop, src/interface/seqalign_cuda.c:181,286-289,293) */
	r->show_progress = !no_progress && !quiet;
	if (r->show_progress) {
		sa_hip_set_progress(progress_line, NULL);
		progress_line(0.0, NULL);
	}
	verb("Devices: %d (%s)", sa_hip_device_count(), sa_hip_device_name(0) ? sa_hip_device_name(0) : "none");
	if (!(r->o.query ? run_search(r) : r->device_deflate ? run_tile_job(r) : r->no_matrix ? run_only(r) : run_host_matrix(r)))
		return 1;
	if (r->o.query) { /* a search has one selection, the hits, and one writer */
		if (!trace_hits(r) || !write_search(r))
			return 1;
	} else if (!pass_neighbors(r) || !write_neighbors(r) || !trace_alignments(r) || !pass_quantiles(r) || !pass_edges(r) || !write_edges(r) ||
	    !pass_linkage(r) || !write_linkage(r) || !write_quantiles_and_quantity(r))
		return 1;
	if (r->o.benchmark)
		report(r);
	release(r);
	/* everything is written and closed: leave without the runtime's teardown (device reset, queue and signal
	 * destruction: ~0.15 s that nothing waits for) */
	fflush(NULL);
	if (getenv("SA_CLI_CLEAN_EXIT")) /* (a profiler that writes its files from an exit handler: rocprofv3) */
		return 0;
	_exit(0);
}
