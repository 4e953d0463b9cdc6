/* sa_search_run.h -- what every one-call search form (sa_hip_search, _norm, _pid, _above, _strands, _above_strands, _fit) needs
 * around its own launches, once: the store and device checks, the context, the batch rule, the device buffers, the stream, the
 * phase clock, and the stage that makes a batch's rectangles.  Header-only; the byte and batch arithmetic is in
 * sa_search_batch_core.h, which the host compiles as well.  DESIGN 4.22 describes the driver.
 *
 * A form reads: its own argument checks, with sa_run_stores_* and sa_run_device_check between them where the form has them;
 * SearchRun::adopt of its context; what must exist before the free memory is read (payload scratch); SearchRun::size or
 * RectStage::begin; its own buffers; SearchRun::start; SearchRun::each_batch over a body that stamps the clock before every phase;
 * the mapping from the clock's totals to the sa_hip_last_* values. */
#ifndef SA_SEARCH_RUN_H
#define SA_SEARCH_RUN_H

#include <algorithm>
#include <cstdint>
#include <deque>
#include <vector>

#include "sa_ctx.h"
#include "sa_search_batch_core.h"
#include "sa_strands_core.h"

/* ---- the checks that every form makes, each at its own place among the form's own --------------------------------------------- */
static inline bool sa_run_stores_not_empty(const char *who, struct sa_input db, struct sa_input queries)
{
	if (db.num < 1 || queries.num < 1) {
		sa_set_error("%s: empty store (%d database sequences, %d queries; min: 1 each)", who, db.num, queries.num);
		return false;
	}
	return true;
}

static inline bool sa_run_stores_not_null(const char *who, struct sa_input db, struct sa_input queries)
{
	if (!db.seqs || !db.meta || !queries.seqs || !queries.meta) {
		sa_set_error("%s: null sequence store", who);
		return false;
	}
	return true;
}

static inline bool sa_run_device_check()
{
	if (sa_hip_device_count() <= 0) {
		sa_set_error("No HIP devices available; libseqalign_hip has no CPU fallback");
		return false;
	}
	return true;
}

namespace { /* internal linkage: every translation unit that drives a form has its own copy, the library exports none of it */

struct DevBuf {
	void *p = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	~DevBuf() { (void)hipFree(p); }
	bool alloc(const char *who, size_t want, const char *what)
	{
		if (hipMalloc(&p, std::max<size_t>(want, 8)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			sa_set_error("%s: %s (%.2f GiB) does not fit the device's memory", who, what, (double)want / (double)(1 << 30));
			return false;
		}
		bytes = want;
		return true;
	}
};

/* ---- the phase clock ----------------------------------------------------------------------------------------------------------
 * stamp(s, phase) records an event on the stream and names the phase that the work enqueued after it belongs to; SA_PH_END says
 * that what follows (copies to the host) is nobody's.  After the stream has been synchronised, collect() adds every interval
 * between consecutive stamps to its phase's total and starts over: a batch may collect more than once.  A phase that does not run
 * is not stamped and stays at exactly 0.  The events are a fixed pool, created once per call. */
enum SaPhase { SA_PH_ALIGN, SA_PH_GATHER, SA_PH_QUANTITY, SA_PH_FOLD, SA_PH_SELECT, SA_PH_FILL, SA_PH_STRAND_TAKE, SA_PH_FIT, SA_PH_END, SA_PH_COUNT };

struct PhaseClock {
	enum { POOL = 12 }; /* the most stamps between two collects: nine, a batch of sa_hip_search_strands */
	hipEvent_t ev[POOL] = {};
	SaPhase phase[POOL] = {};
	int used = 0;
	double seconds[SA_PH_COUNT] = {};
	bool create()
	{
		for (hipEvent_t &e : ev)
			SA_HIP_CHECK(hipEventCreate(&e), return false);
		return true;
	}
	void destroy()
	{
		for (hipEvent_t &e : ev) {
			if (e)
				(void)hipEventDestroy(e);
			e = nullptr;
		}
	}
	/* the next event, for a callee that records it itself (sa_search_range_launch: between alignment and gather); NULL +
	 * sa_set_error when the pool is used up, which the caller checks */
	hipEvent_t hand_out(SaPhase after)
	{
		if (used >= POOL) {
			sa_set_error("phase clock: more than %d stamps between two collects", (int)POOL);
			return nullptr;
		}
		phase[used] = after;
		return ev[used++];
	}
	bool stamp(hipStream_t s, SaPhase after)
	{
		hipEvent_t e = hand_out(after);
		if (!e)
			return false;
		SA_HIP_CHECK(hipEventRecord(e, s), return false);
		return true;
	}
	bool collect()
	{
		for (int t = 0; t + 1 < used; t++) {
			if (phase[t] == SA_PH_END)
				continue;
			float ms = 0.f;
			SA_HIP_CHECK(hipEventElapsedTime(&ms, ev[t], ev[t + 1]), return false);
			seconds[phase[t]] += (double)ms * 1e-3;
		}
		used = 0;
		return true;
	}
	double operator[](SaPhase p) const { return seconds[p]; }
};

struct Sync { /* the stream and the clock's events; drain() synchronises the stream before it goes */
	hipStream_t s = nullptr;
	PhaseClock clock;
	void drain()
	{
		if (s) {
			(void)hipStreamSynchronize(s);
			(void)hipStreamDestroy(s);
			s = nullptr;
		}
		clock.destroy();
	}
};

/* ---- one call of a one-call form ------------------------------------------------------------------------------------------------
 * Owns the context, every device buffer of the call and the stream, and lets them go in the one order that is right: the stream is
 * drained, then the buffers are freed, then the context is destroyed -- whatever the order in which a form asked for them. */
struct SearchRun {
	const char *who;
	sa_ctx *ctx = nullptr;
	int64_t n = 0, m = 0; /* database sequences, queries (of one strand) */
	int32_t nqb = 0, batches = 0;
	std::deque<DevBuf> bufs;
	Sync sy;
	explicit SearchRun(const char *w) : who(w) {}
	~SearchRun()
	{
		sy.drain();
		while (!bufs.empty()) /* (the last first, as locals go) */
			bufs.pop_back();
		sa_ctx_destroy(ctx);
	}
	/* the context that sa_ctx_create_search / _strands returned (NULL: it has said why) */
	bool adopt(sa_ctx *c, struct sa_input db, struct sa_input queries)
	{
		ctx = c;
		n = db.num;
		m = queries.num;
		return c != nullptr;
	}
	/* the batch rule (sa_search_batch_core.h); whatever the call allocates outside its batches exists by now */
	bool size(int64_t per_query)
	{
		size_t free_b = 0, total_b = 0;
		SA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b), return false);
		nqb = sa_batch_queries(m, sa_batch_budget(free_b, ctx->env.search_batch_bytes), per_query);
		return true;
	}
	/* the largest of f(q0, nq) over the batches: what a buffer that every batch reuses must hold */
	template <class F> size_t largest(F f) const
	{
		size_t most = 0;
		for (int64_t q0 = 0; q0 < m; q0 += nqb)
			most = std::max<size_t>(most, f((int32_t)q0, sa_batch_nq(m, nqb, q0)));
		return most;
	}
	template <class T> bool alloc(T *&out, size_t bytes, const char *what)
	{
		DevBuf &b = spare();
		if (!b.alloc(who, bytes, what))
			return false;
		out = static_cast<T *>(b.p);
		return true;
	}
	DevBuf &spare() /* an empty buffer of the call's, for a form that sizes it later */
	{
		bufs.emplace_back();
		return bufs.back();
	}
	bool start() /* after the buffers: the stream and the clock */
	{
		SA_HIP_CHECK(hipStreamCreateWithFlags(&sy.s, hipStreamNonBlocking), return false);
		return sy.clock.create();
	}
	bool stamp(SaPhase after) { return sy.clock.stamp(sy.s, after); }
	bool sync() /* (on a stream that a body has drained already this returns at once) */
	{
		SA_HIP_CHECK(hipStreamSynchronize(sy.s), return false);
		return sy.clock.collect();
	}
	/* body(q0, nq) for every batch in order, the stream synchronised after each (the next batch reuses the buffers) */
	template <class F> bool each_batch(F body)
	{
		for (int64_t q0 = 0; q0 < m; q0 += nqb) {
			if (!body(q0, sa_batch_nq(m, nqb, q0)) || !sync())
				return false;
			batches++;
		}
		return true;
	}
};

/* ---- the rectangles of a batch ----------------------------------------------------------------------------------------------------
 * norm: normalised scores; pid_denom: percent identity; neither: raw scores only (value() is then raw()).  strands: the context is
 * a strands context; both halves are made and folded in place, so raw() / value() hold the better strand and bits() says which.
 * Stream order of launch(): forward range, rows; reverse range (rows M + q0 ..) through the same range buffer, rows; denominators
 * at q0 == 0; normalise forward, then reverse; fold.  Under percent identity the identity sweep(s) stand for all before the fold. */
struct RectStage {
	SearchRun &run;
	const struct sa_norm *norm;
	const int32_t *pid_denom;
	const bool strands, quantity, aligned;
	void *d_range = nullptr;
	int32_t *d_den = nullptr, *d_rect = nullptr, *d_rrev = nullptr, *d_vrect = nullptr, *d_vrev = nullptr;
	uint64_t *d_bits = nullptr;
	std::vector<int32_t> h_den;
	RectStage(SearchRun &r, const struct sa_norm *nm, const int32_t *pid, bool st)
		: run(r), norm(nm), pid_denom(pid), strands(st), quantity(nm || pid), aligned(!pid)
	{
	}
	int32_t *raw() const { return d_rect; }
	int32_t *value() const { return quantity ? d_vrect : d_rect; }
	uint64_t *bits() const { return d_bits; }
	size_t dens() const { return (size_t)(run.n + (strands ? 2 : 1) * run.m); }
	/* sizes the batches of the call (`tail`: sa_search_batch_core.h) and allocates what the stage needs; two_names: the forward
	 * rectangles are called so (sa_hip_search_strands) */
	bool begin(int64_t tail, bool two_names = false)
	{
		sa_ctx *ctx = run.ctx;
		/* the identity sweep's payload scratch is the context's and is allocated before the free memory is read, as sa_hip_identity does it */
		if (pid_denom && !sa_identity_payload_scratch(ctx))
			return false;
		const struct sa_batch_form form = { aligned, quantity, strands, tail };
		if (!run.size(sa_batch_per_query(run.n, run.m, form)))
			return false;
		/* (the reverse half begins M queries later: its range is the longer one) */
		const size_t range_bytes =
			aligned ? run.largest([&](int32_t q0, int32_t nq) { return sa_search_scratch_bytes(ctx, strands ? (int32_t)run.m + q0 : q0, nq); }) : 0;
		const size_t rect_bytes = sizeof(int32_t) * (size_t)run.nqb * (size_t)run.n;
		if ((aligned && !run.alloc(d_range, range_bytes, "the packed range of a query batch")) ||
		    (norm && !run.alloc(d_den, sizeof(int32_t) * dens(), "the denominators")) ||
		    !run.alloc(d_rect, rect_bytes, two_names ? "the forward rectangle of a query batch" : "the rectangle of a query batch") ||
		    (strands && !run.alloc(d_rrev, rect_bytes, "the reverse rectangle of a query batch")) ||
		    (quantity && !run.alloc(d_vrect, rect_bytes, two_names ? "the forward value rectangle of a query batch" : "the value rectangle of a query batch")) ||
		    (quantity && strands && !run.alloc(d_vrev, rect_bytes, "the reverse value rectangle of a query batch")) ||
		    (strands && !run.alloc(d_bits, sizeof(uint64_t) * (size_t)run.nqb * (size_t)sa_strand_words(run.n), "the strand bitmap of a query batch")))
			return false;
		h_den.resize(norm && norm->denominators ? dens() : 0);
		return true;
	}
	/* the range of queries [q, q + nq) and its rows into `rect`; the event between the two is the clock's */
	bool range(int32_t q, int32_t nq, int32_t *rect)
	{
		if (!run.stamp(SA_PH_ALIGN))
			return false;
		hipEvent_t mid = run.sy.clock.hand_out(SA_PH_GATHER);
		return mid && sa_search_range_launch(run.ctx, q, nq, rect, d_range, run.sy.s, mid) == 0;
	}
	bool launch(int64_t q0, int32_t nq)
	{
		sa_ctx *ctx = run.ctx;
		hipStream_t s = run.sy.s;
		const int32_t n = (int32_t)run.n, qf = (int32_t)q0, qr = (int32_t)(run.m + q0);
		int32_t *const vf = value(), *const vr = quantity ? d_vrev : d_rrev;
		if (aligned) {
			if (!range(qf, nq, d_rect) || (strands && !range(qr, nq, d_rrev)))
				return false;
			if (norm) {
				if (!run.stamp(SA_PH_QUANTITY))
					return false;
				if (q0 == 0) { /* once per call */
					SA_HIP_CHECK(sa_denominators_launch(ctx, norm->source, d_den, s), return false);
				}
				if (sa_normalize_rect_launch(d_rect, n, qf, nq, d_den, norm->rule, vf, s) != 0 ||
				    (strands && sa_normalize_rect_launch(d_rrev, n, qr, nq, d_den, norm->rule, vr, s) != 0))
					return false;
			}
		} else {
			const struct sa_identity_out fwd = { d_rect, nullptr, nullptr, vf, *pid_denom }, rev = { d_rrev, nullptr, nullptr, vr, *pid_denom };
			if (!run.stamp(SA_PH_QUANTITY) || !sa_identity_rect(run.who, ctx, qf, nq, &fwd, s) || (strands && !sa_identity_rect(run.who, ctx, qr, nq, &rev, s)))
				return false;
		}
		if (strands) { /* in place: the folded values replace the forward values, the folded raw scores the forward raw scores */
			int32_t *const sf = quantity ? d_rect : nullptr;
			if (!run.stamp(SA_PH_FOLD) || sa_strand_fold_launch(vf, vr, sf, quantity ? d_rrev : nullptr, n, nq, vf, sf, d_bits, s) != 0)
				return false;
		}
		return true;
	}
	/* among the copies of the first batch: the denominators towards the host, once per call */
	bool copy_denominators(int64_t q0)
	{
		if (q0 == 0 && !h_den.empty()) {
			SA_HIP_CHECK(hipMemcpyAsync(h_den.data(), d_den, sizeof(int32_t) * h_den.size(), hipMemcpyDeviceToHost, run.sy.s), return false);
		}
		return true;
	}
	void publish_denominators() const /* after the last batch */
	{
		if (!h_den.empty())
			std::copy(h_den.begin(), h_den.end(), norm->denominators);
	}
};

} // namespace

#endif /* SA_SEARCH_RUN_H */
