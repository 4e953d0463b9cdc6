/* tests/host_c/limits_sweep.cpp -- TEST HARNESS (not part of the product library).
 *
 * Sweeps the product's sa_kernel_limits (sequencealigner_amd/csrc/sa_limits.cpp) over a grid of scorings and store
 * length ranges and checks what must hold between its answers; tests/test_limits_host.py builds it with
 * g++ -fsanitize=address,undefined (a signed overflow anywhere in the limits arithmetic fails the run) and runs it on
 * the CPU.
 *
 *   limits_sweep <matrix>...                  the grid: methods x gaps 0..60 x shortest 1..32 x longest 8..5000
 *   limits_sweep --print <method> <matrix> <gap_pen> <gap_open> <gap_ext> <max_len> <min_len>     one `limits:` line and the
 *                                                                                         `shapes:` line (sa_shapes.h)
 *   limits_sweep --print <method> <matrix> ... <min_len> --sub FILE      the same for a table given as data: FILE holds 576
 *                                                                       integers, used in place of the named matrix's table
 *                                                                       (<matrix> may then be "-")
 *
 * Exit status 0 = every property held. */
#include <algorithm>
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sequencealigner_amd/csrc/sa_plan.h"

static long g_fail = 0, g_calls = 0, g_admitted = 0;
#define CHECK(cond, ...)                                          \
	do {                                                      \
		if (!(cond)) {                                    \
			if (g_fail++ < 20) {                      \
				fprintf(stderr, "CHECK FAILED %s: ", #cond); \
				fprintf(stderr, __VA_ARGS__);     \
				fprintf(stderr, "\n");            \
			}                                         \
		}                                                 \
	} while (0)

static SaPlanInputs inputs_of(const SaKernelLimits &L, const sa_scoring &sc, int32_t min_len)
{
	SaPlanInputs in; /* as sa_plan_inputs (sa_context.hip) fills it: what sa_pk_base / sa_pk_delta read */
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
	return in;
}

/* one (scoring, longest): every shortest length 32 .. 1, the answers compared with those of the next longer shortest */
static void sweep_min_len(const sa_scoring &sc, int32_t max_len, const char *tag)
{
	int64_t smax = INT32_MIN;
	for (int k = 0; k < SA_SUB_DIM * SA_SUB_DIM; k++)
		smax = std::max<int64_t>(smax, sc.sub[k]);
	SaKernelLimits prev;
	bool have_prev = false;
	for (int32_t min_len = std::min<int32_t>(32, max_len); min_len >= 1; min_len--) {
		const SaKernelLimits L = sa_kernel_limits(sc, max_len, min_len, false, false, false);
		g_calls++;
		CHECK(L.pk_kmax >= 0 && L.pk_kmax <= SA_PK_KMAX, "%s max %d min %d: pk_kmax %d", tag, max_len, min_len, L.pk_kmax);
		CHECK(L.pk16_kmax == 0 || (L.pk16_kmax >= SA_PK_K16_MIN && L.pk16_kmax <= SA_PK16_KMAX), "%s max %d min %d: pk16_kmax %d", tag, max_len,
		      min_len, L.pk16_kmax);
		CHECK(L.pk16_f16_kmax <= L.pk16_kmax && L.pk16_f16_kmax <= SA_PK16_F16_KMAX, "%s max %d min %d: f16 %d above pk16 %d", tag, max_len, min_len,
		      L.pk16_f16_kmax, L.pk16_kmax);
		CHECK(L.pk16_kmax == 0 || L.pk_kmax == SA_PK_KMAX, "%s max %d min %d: pk16 %d with pk %d", tag, max_len, min_len, L.pk16_kmax, L.pk_kmax);
		CHECK(L.sys_ok || L.pk_kmax == 0, "%s max %d min %d: packed classes without the s32 family", tag, max_len, min_len);
		if (have_prev) { /* prev = the same store with a LONGER shortest sequence: it admits at least as much */
			CHECK(L.pk_kmax <= prev.pk_kmax, "%s max %d: pk_kmax %d at shortest %d, %d at %d", tag, max_len, L.pk_kmax, min_len, prev.pk_kmax, min_len + 1);
			CHECK(L.pk16_kmax <= prev.pk16_kmax, "%s max %d: pk16_kmax %d at shortest %d, %d at %d", tag, max_len, L.pk16_kmax, min_len, prev.pk16_kmax,
			      min_len + 1);
			CHECK(L.pk16_f16_kmax <= prev.pk16_f16_kmax, "%s max %d: pk16_f16_kmax %d at shortest %d, %d at %d", tag, max_len, L.pk16_f16_kmax, min_len,
			      prev.pk16_f16_kmax, min_len + 1);
			CHECK(L.sys_ok == prev.sys_ok, "%s max %d: sys_ok depends on the shortest sequence", tag, max_len);
		}
		prev = L;
		have_prev = true;
		if (!L.pk_kmax)
			continue;
		/* every admitted class: one frame above BASE plus the largest profile entry stays inside the form's range */
		const SaPlanInputs in = inputs_of(L, sc, min_len);
		const int64_t pmax = smax + L.pk_pconst - (sc.method == SA_METHOD_GA ? L.pk_q : 0);
		CHECK(pmax >= 0 && L.pk_floor >= 0, "%s: pmax %" PRId64 " floor %d", tag, pmax, L.pk_floor);
		for (int k = 1; k <= L.pk_kmax; k++) {
			const int64_t top = (int64_t)sa_pk_base(in, 8, k) + sa_pk_delta(in, 8, k) + pmax;
			CHECK(sa_pk_delta(in, 8, k) > 0 && top <= SA_PK_F16_MAX, "%s max %d min %d: 8-lane K %d reaches %" PRId64, tag, max_len, min_len, k, top);
			g_admitted++;
		}
		for (int k = SA_PK_K16_MIN; k <= L.pk16_kmax; k++) {
			const int64_t top = (int64_t)sa_pk_base(in, 16, k) + sa_pk_delta(in, 16, k) + pmax;
			const int64_t limit = k <= L.pk16_f16_kmax ? SA_PK_F16_MAX : 65535;
			CHECK(sa_pk_delta(in, 16, k) > 0 && top <= limit, "%s max %d min %d: 16-lane K %d reaches %" PRId64 " of %" PRId64, tag, max_len, min_len, k,
			      top, limit);
			g_admitted++;
		}
	}
}

static const int32_t MAX_LENS[] = { 8, 9, 31, 64, 192, 193, 500, 1000, 1023, 1024, 1025, 2048, 3000, 5000 };

static void sweep_scoring(sa_scoring sc, const char *matrix)
{
	char tag[128];
	for (int32_t max_len : MAX_LENS) {
		snprintf(tag, sizeof(tag), "%s %s pen %d open %d ext %d", sa_method_name(sc.method), matrix, sc.gap_pen, sc.gap_opn, sc.gap_ext);
		sweep_min_len(sc, max_len, tag);
	}
}

int main(int argc, char **argv)
{
	if (argc >= 9 && !strcmp(argv[1], "--print")) {
		sa_scoring sc{};
		sc.method = sa_method_parse(argv[2]);
		const bool own_table = argc >= 11 && !strcmp(argv[9], "--sub");
		if (sc.method < 0 || (!(own_table && !strcmp(argv[3], "-")) && sa_matrix_load(argv[3], sc.lut, sc.sub))) {
			fprintf(stderr, "%s\n", sa_last_error());
			return 2;
		}
		if (own_table) {
			FILE *f = fopen(argv[10], "r");
			int got = 0;
			long long v;
			while (f && got < SA_SUB_DIM * SA_SUB_DIM && fscanf(f, "%lld", &v) == 1 && v >= INT32_MIN && v <= INT32_MAX)
				sc.sub[got++] = (int32_t)v;
			const bool more = f && fscanf(f, "%lld", &v) == 1;
			if (f)
				fclose(f);
			if (got != SA_SUB_DIM * SA_SUB_DIM || more) {
				fprintf(stderr, "limits_sweep --sub %s: %d int32 values read, %d expected and no more\n", argv[10], got, SA_SUB_DIM * SA_SUB_DIM);
				return 2;
			}
		}
		sc.gap_pen = -atoi(argv[4]);
		sc.gap_opn = -atoi(argv[5]);
		sc.gap_ext = -atoi(argv[6]);
		const SaKernelLimits L = sa_kernel_limits(sc, atoi(argv[7]), atoi(argv[8]), false, false, false);
		printf("limits: sys_ok %d pk_kmax %d pk16_kmax %d (f16 up to %d) chunk cap %d\n", (int)L.sys_ok, L.pk_kmax, L.pk16_kmax, L.pk16_f16_kmax,
		       L.pk_chunk_cap);
		/* the class geometry of sa_shapes.h, so that the tests' own copies of it cannot drift away unnoticed */
		printf("shapes: pk_kmax %d pk16_kmin %d pk16_kmax %d pk16_f16_kmax %d pk_wpb %d sys_chunk %d long_w %d\n", SA_PK_KMAX, SA_PK_K16_MIN,
		       SA_PK16_KMAX, SA_PK16_F16_KMAX, SA_PK_WPB, SA_SYS_CHUNK, (int)SA_SYS_LONG_W);
		return 0;
	}
	if (argc < 2) {
		fprintf(stderr, "usage: limits_sweep <matrix>... | --print method matrix gap_pen gap_open gap_ext max_len min_len [--sub FILE]\n");
		return 2;
	}
	static const int EXT[] = { 0, 1, 2, 3, 4, 5, 8, 11, 16, 30, 60 };
	static const int32_t EXTREME[] = { 61, 127, 128, 4096, 4097, 16700, 16800, 65535, 1 << 20, INT32_MAX / 2, INT32_MAX - 1, INT32_MAX };
	for (int a = 1; a < argc; a++) {
		sa_scoring sc{};
		if (sa_matrix_load(argv[a], sc.lut, sc.sub)) {
			fprintf(stderr, "%s\n", sa_last_error());
			return 2;
		}
		for (int method : { SA_METHOD_NW, SA_METHOD_GA, SA_METHOD_SW }) {
			sc.method = method;
			sc.gap_pen = sc.gap_opn = sc.gap_ext = 0;
			if (method == SA_METHOD_NW) {
				for (int g = 0; g <= 60; g++) {
					sc.gap_pen = -g;
					sweep_scoring(sc, argv[a]);
				}
				for (int32_t g : EXTREME) { /* (gaps are stored negated: the largest magnitude is -INT32_MAX) */
					sc.gap_pen = -g;
					sweep_scoring(sc, argv[a]);
				}
				continue;
			}
			for (int o = 0; o <= 60; o++)
				for (int e : EXT) {
					sc.gap_opn = -o;
					sc.gap_ext = -e;
					sweep_scoring(sc, argv[a]);
				}
			for (int32_t o : EXTREME)
				for (int32_t e : { 0, 1, 60, 16700, INT32_MAX }) {
					sc.gap_opn = -o;
					sc.gap_ext = -e;
					sweep_scoring(sc, argv[a]);
					sc.gap_opn = -e;
					sc.gap_ext = -o;
					sweep_scoring(sc, argv[a]);
				}
		}
	}
	printf("limits_sweep: %ld calls, %ld admitted classes checked, %ld failures\n", g_calls, g_admitted, g_fail);
	return g_fail ? 1 : 0;
}
