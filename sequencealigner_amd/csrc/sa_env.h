/* sa_env.h -- every environment switch of libseqalign_hip.so in ONE table (README lists them).
 *
 * All of them are diagnostics, experiments or test hooks; none is needed to use the library.  The table is read
 * once per context (sa_ctx_create) and once per sa_hip_align / sa_hip_memory call -- never per launch -- so a test may
 * change a switch between two contexts of one process. */
#ifndef SA_ENV_H
#define SA_ENV_H

struct SaEnv {
	/* kernel-family selection (parity tests A/B the families against each other) */
	bool force_generic = false; /* SA_HIP_FORCE_GENERIC : pair-per-wave kernels for everything                     */
	bool no_pk = false;         /* SA_HIP_NO_PK         : no packed-u16 kernels (the s32 systolic classes run)      */
	bool no_pk16 = false;       /* SA_HIP_NO_PK16       : no 16-lane packed kernels                                 */
	bool no_sort = false;       /* SA_HIP_NO_SORT       : row streams in store order (no arranged copies)           */
	bool no_tokens = false;     /* SA_HIP_NO_TOKENS     : no pre-built token streams: every packed tile derives its tokens   */
	bool no_remainder = false;  /* SA_HIP_NO_REMAINDER  : no half / quarter tiles: a pair's last rows are one store-order partial tile */
	/* launch structure */
	int chunk = 0;               /* SA_HIP_CHUNK=n        : fixed row-stream length (1..32)                         */
	int stagger = 0;             /* SA_HIP_STAGGER=n      : start delay per wave slot (sleep periods)               */
	/* host delivery */
	bool no_pin = false;    /* SA_HIP_NO_PIN    : never page-lock the destination                                   */
	bool no_direct = false; /* SA_HIP_NO_DIRECT : batched copies instead of direct stores into a locked packed matrix */
	bool no_shells = false; /* SA_HIP_NO_SHELLS : host scatter for the full layout                                  */
	/* sa_hip_align */
	int devices = 0; /* SA_HIP_DEVICES=n : use the first n visible devices                                           */
	int split = 0;   /* SA_HIP_SPLIT=n   : n slices even when fewer devices are visible (testing aid)                */
	int gather = -1; /* SA_HIP_GATHER=0/1: multi-device path through dense shares + RCCL all-gather (-1: default)    */
	int tiles_split = 0; /* SA_HIP_TILES_SPLIT=n: sa_hip_tiles_begin deals the column blocks over n jobs on device 0 (testing aid) */
	/* traceback (sa_traceback.hip) */
	long long trace_batch_bytes = 0; /* SA_HIP_TRACE_BATCH_BYTES=n : cap on the decision scratch of one batch of pairs (0: from the free device memory) */
	/* percent identity (sa_identity.hip) */
	long long identity_batch_bytes = 0; /* SA_HIP_IDENTITY_BATCH_BYTES=n : cap on the device buffers of one column range of sa_hip_identity (0: from the free device memory) */
	/* search (sa_search_run.h) */
	long long search_batch_bytes = 0; /* SA_HIP_SEARCH_BATCH_BYTES=n : cap on the device buffers of one query batch of every one-call search form (0: from the free device memory) */
	/* diagnostics */
	bool verbose = false;             /* SA_HIP_VERBOSE                                                               */
	bool stamps = false;              /* SA_HIP_STAMPS : per-tile clocks of every launch (synchronous)                */
	const char *stamps_dump = nullptr; /* SA_HIP_STAMPS_DUMP=<file> : raw stamp words                                 */
	bool ztrace = false;              /* SA_HIP_ZTRACE : the tile walk (sa_deflate.hip) prints what every block / batch cost  */
};

/* a fresh snapshot of the process environment */
SaEnv sa_env_read();

#endif /* SA_ENV_H */
