// Host side of a device-resident nested-sampling run: mcalf_nested_open / _advance / _finish / _read / _last_round / _close.
// The live set and the dead rows stay in HBM (NsRun, host_ctx.h); a round is the book-keeping kernels of ns_round_kernels.hip
// around one polling call of the replacement step (host_ns.cpp: run_ns) on device rows, and ONE copy of the round record into
// page-locked memory.  The evidence is ns_evidence.h's.  A multi-device context runs everything on its first device entry.
#include <cmath>

#include "ns_round_args.h"
#include "host_ctx.h"

static_assert(sizeof(mcalf_nested_opts) == 40, "mcalf_nested_opts is 40 bytes");
static_assert(sizeof(mcalf_nested_state_t) == 80, "mcalf_nested_state_t is 80 bytes");

namespace {

constexpr int64_t kNsrMaxStateBytes = 4LL << 30;      // largest state (live and dead rows with their logL) a run may keep
constexpr char kNsrLaunch[] = "hipLaunchKernel(nsr_kernel_ptr(k), dim3(grid), dim3(block), args, lds, stream)";

// The context that holds the run: a multi-device parent's first entry.
mcalf_ctx* holder(mcalf_ctx* ctx) { return is_multi(ctx) ? ctx->subs[0] : ctx; }

// An error of the holder, reported on the context the caller holds.
int lift(mcalf_ctx* ctx, mcalf_ctx* w, int rc) {
    if (rc && w != ctx) return set_err(ctx, rc, "device entry 0 (HIP device %d): %s", w->device, w->err.c_str());
    return rc;
}

int launch_nsr(mcalf_ctx* w, NsrKernel k, const NsrArgs& a, unsigned grid, unsigned block, size_t lds = 0) {
    void* argv[] = {(void*)&a};
    const hipError_t e = hipLaunchKernel(nsr_kernel_ptr(k), dim3(grid), dim3(block), argv, lds, w->stream);
    return e == hipSuccess ? MCALF_OK : set_err(w, MCALF_ERR_HIP, "%s failed: %s", kNsrLaunch, hipGetErrorString(e));
}

size_t tri_doubles(const mcalf_ctx* w) { return (size_t)w->ndim * ((size_t)w->ndim + 1) / 2; }

NsrArgs round_args(mcalf_ctx* w) {
    NsRun& s = w->nsrun;
    NsrArgs a = {};
    a.UL = s.UL; a.LL = s.LL; a.UD = s.UD; a.LD = s.LD; a.rank = s.rank; a.order = s.order; a.dying = s.dying; a.pick = s.pick;
    a.meanpart = s.meanpart; a.covpart = s.covpart; a.tri = s.tri; a.var = s.var; a.D = s.D; a.U0 = s.U0; a.Lmin = s.Lmin; a.sid = s.sid;
    a.Un = s.Un; a.Ln = s.Ln; a.status = s.status; a.nevals = s.nevals_row; a.rec = s.rec;
    a.seed = s.opts.seed; a.round = (uint64_t)s.rounds; a.ndead = s.ndead;
    a.nlive = (int)s.nlive; a.ndim = w->ndim; a.K = s.opts.batch;
    a.chol_in_lds = tri_doubles(w) * sizeof(double) <= kNsrCholLds ? 1 : 0;
    return a;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// The time stamp `i` of a timed round.
int stamp(mcalf_ctx* w, int i) {
    NsRun& s = w->nsrun;
    if (!s.timing) return MCALF_OK;
    if (!s.ev_t[i]) HIP_TRY(w, hipEventCreate(&s.ev_t[i]));
    HIP_TRY(w, hipEventRecord(s.ev_t[i], w->stream));
    return MCALF_OK;
}

int grow_state(mcalf_ctx* w, int64_t nlive, const mcalf_nested_opts& o) {
    NsRun& s = w->nsrun;
    const size_t n = (size_t)nlive, ndim = (size_t)w->ndim, K = (size_t)o.batch, md = (size_t)o.max_dead, tri = tri_doubles(w);
    int rc;
    if ((rc = grow(w, s.UL, n * ndim)) || (rc = grow(w, s.LL, n)) || (rc = grow(w, s.UD, md * ndim)) || (rc = grow(w, s.LD, md)) ||
        (rc = grow(w, s.meanpart, (size_t)kNsrChunks * ndim)) || (rc = grow(w, s.covpart, (size_t)kNsrChunks * tri)) || (rc = grow(w, s.tri, tri)) ||
        (rc = grow(w, s.var, ndim)) || (rc = grow(w, s.D, ndim * ndim)) ||
        // (the rows of the replacement call: the initial points are one of nlive rows, a round's has K < nlive)
        (rc = grow(w, s.U0, n * ndim)) || (rc = grow(w, s.Lmin, n)) || (rc = grow(w, s.Un, n * ndim)) || (rc = grow(w, s.Ln, n)) ||
        (rc = grow(w, s.rank, n)) || (rc = grow(w, s.order, n)) || (rc = grow(w, s.dying, K)) || (rc = grow(w, s.pick, K)) ||
        (rc = grow(w, s.status, n)) || (rc = grow(w, s.nevals_row, n)) || (rc = grow(w, s.moves, n)) || (rc = grow(w, s.sid, n)) ||
        (rc = grow(w, s.rec, K + kNsrRecWords)) || (rc = grow(w, s.h_rec, K + kNsrRecWords)))
        return rc;
    s.keys.resize(K);
    return MCALF_OK;
}

double word_double(uint64_t v) { double d; std::memcpy(&d, &v, sizeof d); return d; }

int open_run(mcalf_ctx* w, const double* U0, int64_t nlive, const mcalf_nested_opts& o) {
    NsRun& s = w->nsrun;
    HIP_TRY(w, hipSetDevice(w->device));
    begin_call(w, MCALF_PATH_HOST_STAGED, is_pinned_host(U0), false);
    int rc;
    if ((rc = grow_state(w, nlive, o))) return rc;
    const size_t n = (size_t)nlive, ndim = (size_t)w->ndim;
    const hipStream_t st = w->stream;
    // the initial points: the replacement call's checked start (nmoves = 0) without a constraint
    std::vector<double> minus_inf(n, -INFINITY);
    HIP_TRY(w, hipMemcpyAsync(s.U0, U0, n * ndim * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(w, hipMemcpyAsync(s.Lmin, minus_inf.data(), n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(w, hipMemsetAsync(s.sid, 0, n * sizeof(uint64_t), st));
    HIP_TRY(w, hipMemsetAsync(s.D, 0, ndim * ndim * sizeof(double), st));
    const NsRows rows = {s.U0, s.Lmin, s.D, s.sid, s.UL, nullptr, s.LL, s.status, s.nevals_row, s.moves};
    const mcalf_slice_opts so = {0, 0, w->ndim, 0, o.seed};
    if ((rc = run_ns(w, rows, nlive, so, st, true))) return rc;
    s.opts = o; s.nlive = nlive; s.ndead = 0; s.rounds = 0;
    if ((rc = launch_nsr(w, kNsrInit, round_args(w), blocks_of(nlive, kNsrBlock), kNsrBlock))) return rc;
    std::vector<double> L(n);
    HIP_TRY(w, hipMemcpyAsync(L.data(), s.LL, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(w, hipStreamSynchronize(st));
    s.nevals = nlive; s.unfinished = 0; s.rows_launched = w->ns_stats.rows_launched;
    s.max_key = -INFINITY;
    for (double l : L) s.max_key = std::max(s.max_key, ns_key(l));
    s.reason = MCALF_NESTED_BUDGET; s.have_last = false; s.timed = false;
    s.ev = NsEvidence(); s.logw.clear(); s.host_l.clear();
    s.phase = NsRun::kOpen;
    return MCALF_OK;
}

// One round on the device; the record is in h_rec when it returns.
int issue_round(mcalf_ctx* w) {
    NsRun& s = w->nsrun;
    const NsrArgs a = round_args(w);
    const unsigned K = (unsigned)a.K;
    const size_t lds = a.chol_in_lds ? tri_doubles(w) * sizeof(double) : 0;
    int rc;
    if ((rc = stamp(w, 0)) || (rc = launch_nsr(w, kNsrRank, a, blocks_of(a.nlive, kNsrRankRows), kNsrBlock)) ||
        (rc = stamp(w, 1)) || (rc = launch_nsr(w, kNsrSelect, a, 1, kNsrBlock)) ||
        (rc = stamp(w, 2)) || (rc = launch_nsr(w, kNsrMean, a, kNsrChunks, kNsrWave)) || (rc = launch_nsr(w, kNsrCov, a, kNsrChunks, kNsrBlock)) ||
        (rc = stamp(w, 3)) || (rc = launch_nsr(w, kNsrChol, a, 1, kNsrBlock, lds)) ||
        (rc = stamp(w, 4)) || (rc = launch_nsr(w, kNsrGather, a, K, kNsrWave)) || (rc = stamp(w, 5)))
        return rc;
    const NsRows rows = {s.U0, s.Lmin, s.D, s.sid, s.Un, nullptr, s.Ln, s.status, s.nevals_row, s.moves};
    const mcalf_slice_opts so = {s.opts.nmoves, s.opts.max_steps, w->ndim, 0, s.opts.seed};
    if ((rc = run_ns(w, rows, a.K, so, w->stream, true)) || (rc = stamp(w, 6)) ||
        (rc = launch_nsr(w, kNsrRetire, a, std::min(K, 256u), kNsrBlock)) || (rc = stamp(w, 7)))
        return rc;
    HIP_TRY(w, hipMemcpyAsync(s.h_rec.p, s.rec, ((size_t)K + kNsrRecWords) * sizeof(uint64_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(w, hipStreamSynchronize(w->stream));
    s.have_last = true;
    s.timed = s.timing;
    if (s.timed)
        for (int i = 0; i < 7; ++i) HIP_TRY(w, hipEventElapsedTime(&s.last_ms[i], s.ev_t[i], s.ev_t[i + 1]));
    return MCALF_OK;
}

int advance_run(mcalf_ctx* w, int32_t max_rounds) {
    NsRun& s = w->nsrun;
    HIP_TRY(w, hipSetDevice(w->device));
    begin_call(w, MCALF_PATH_HOST_STAGED, false, false);
    const int64_t K = s.opts.batch;
    for (int32_t done = 0;; ++done) {
        if (s.ev.converged(s.max_key, s.opts.dlogz)) { s.reason = MCALF_NESTED_CONVERGED; return MCALF_OK; }
        if (s.ndead + K + s.nlive > s.opts.max_dead) { s.reason = MCALF_NESTED_FULL; return MCALF_OK; }
        if (done >= max_rounds) { s.reason = MCALF_NESTED_BUDGET; return MCALF_OK; }
        const int rc = issue_round(w);
        if (rc) return rc;
        const uint64_t* rec = s.h_rec.p + K;
        if ((int64_t)rec[kRecNstarts] == 0) { s.reason = MCALF_NESTED_PLATEAU; return MCALF_OK; }
        if ((int64_t)rec[kRecBad] != 0)
            return set_err(w, MCALF_ERR_INVALID, "mcalf_nested_advance: round %lld: %lld replacements came back outside their constraint, the first "
                           "is row %lld; the live and the dead set are those before the round", (long long)s.rounds, (long long)rec[kRecBad],
                           (long long)rec[kRecFirstBad]);
        std::memcpy(s.keys.data(), s.h_rec.p, (size_t)K * sizeof(double));       // (the record's first K words are doubles)
        s.ev.die(s.keys.data(), K, s.nlive, nullptr);
        s.ndead += K; s.rounds += 1;
        s.nevals += (int64_t)rec[kRecNevals]; s.unfinished += (int64_t)rec[kRecUnfinished];
        s.rows_launched += w->ns_stats.rows_launched;
        s.max_key = word_double(rec[kRecMaxKey]);
    }
}

int finish_run(mcalf_ctx* w) {
    NsRun& s = w->nsrun;
    HIP_TRY(w, hipSetDevice(w->device));
    begin_call(w, MCALF_PATH_HOST_STAGED, false, false);
    const NsrArgs a = round_args(w);
    int rc;
    if ((rc = launch_nsr(w, kNsrRank, a, blocks_of(a.nlive, kNsrRankRows), kNsrBlock)) || (rc = launch_nsr(w, kNsrFinal, a, (unsigned)a.nlive, kNsrWave)))
        return rc;
    const size_t nd = (size_t)(s.ndead + s.nlive);
    s.host_l.resize(nd);
    HIP_TRY(w, hipMemcpyAsync(s.host_l.data(), s.LD, nd * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(w, hipStreamSynchronize(w->stream));
    s.ndead += s.nlive;
    s.logw.resize(nd);
    ns_finish(s.host_l.data(), s.ndead, s.nlive, s.opts.batch, s.logw.data(), &s.logZ, &s.H);
    s.phase = NsRun::kFinished;
    return MCALF_OK;
}

int read_run(mcalf_ctx* w, int64_t first, int64_t count, double* cube, double* theta, double* logL, double* logw) {
    NsRun& s = w->nsrun;
    if (count == 0) return MCALF_OK;
    HIP_TRY(w, hipSetDevice(w->device));
    begin_call(w, MCALF_PATH_HOST_STAGED, false, false);
    const size_t ndim = (size_t)w->ndim, n = (size_t)count, f = (size_t)first;
    int rc;
    if (cube) HIP_TRY(w, hipMemcpyAsync(cube, s.UD + f * ndim, n * ndim * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    if (theta) {
        if ((rc = grow(w, s.theta, n * ndim)) || (rc = cube_to_theta(w, s.UD + f * ndim, s.theta, count, w->stream))) return rc;
        HIP_TRY(w, hipMemcpyAsync(theta, s.theta, n * ndim * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    }
    if (logL) HIP_TRY(w, hipMemcpyAsync(logL, s.LD + f, n * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(w, hipStreamSynchronize(w->stream));
    if (logw) std::memcpy(logw, s.logw.data() + f, n * sizeof(double));
    return MCALF_OK;
}

int last_round(mcalf_ctx* w, int32_t* dying, int32_t* pick, double* D, double* lmin) {
    NsRun& s = w->nsrun;
    HIP_TRY(w, hipSetDevice(w->device));
    const size_t K = (size_t)s.opts.batch, ndim = (size_t)w->ndim;
    if (dying) HIP_TRY(w, hipMemcpyAsync(dying, s.dying, K * sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
    if (pick) HIP_TRY(w, hipMemcpyAsync(pick, s.pick, K * sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
    if (D) HIP_TRY(w, hipMemcpyAsync(D, s.D, ndim * ndim * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(w, hipStreamSynchronize(w->stream));
    if (lmin) *lmin = word_double(s.h_rec.p[K + kRecLmin]);
    return MCALF_OK;
}

}  // namespace

extern "C" int mcalf_nested_open(mcalf_ctx* ctx, const double* U0, int64_t nlive, const mcalf_nested_opts* o) {
    constexpr char name[] = "mcalf_nested_open";
    // (the checks of the arguments alone first, as the other samplers order them: they need no context)
    if (!U0) return set_err(ctx, MCALF_ERR_INVALID, "%s: U0 is NULL", name);
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (o->batch < 1 || (int64_t)o->batch >= nlive)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be in [1, nlive), got %d with nlive %lld", name, o->batch, (long long)nlive);
    if (o->nmoves < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nmoves must be >= 0, got %d", name, o->nmoves);
    if (o->max_steps < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: max_steps must be >= 0, got %d", name, o->max_steps);
    if (!(o->dlogz >= 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: dlogz must be >= 0 (0: never stops), got %g", name, o->dlogz);
    if (o->max_dead < nlive + o->batch)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: max_dead must be >= nlive + batch = %lld, got %lld", name, (long long)(nlive + o->batch), (long long)o->max_dead);
    if (nlive > kNsrMaxLive) return set_err(ctx, MCALF_ERR_RANGE, "%s: nlive %lld is above the cap of %lld (the rank is counted)", name, (long long)nlive, (long long)kNsrMaxLive);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the run lives in its unit cube)", name);
    if (ctx->ndim > kNsrCovMaxDim) return set_err(ctx, MCALF_ERR_RANGE, "%s: ndim %d is above the cap of %d (the covariance tile)", name, ctx->ndim, kNsrCovMaxDim);
    const int64_t per = ((int64_t)ctx->ndim + 1) * (int64_t)sizeof(double);
    if (o->max_dead > kNsrMaxStateBytes / per - nlive)
        return set_err(ctx, MCALF_ERR_RANGE, "%s: a state of %lld live and max_dead %lld rows of %d coordinates exceeds the %lld bytes a run may keep on the "
                       "device; the largest max_dead for this run is %lld", name, (long long)nlive, (long long)o->max_dead, ctx->ndim, (long long)kNsrMaxStateBytes,
                       (long long)(kNsrMaxStateBytes / per - nlive));
    mcalf_ctx* w = holder(ctx);
    if (w->nsrun.phase != NsRun::kClosed) return set_err(ctx, MCALF_ERR_INVALID, "%s: a run is already open on this context (mcalf_nested_close ends it)", name);
    return lift(ctx, w, open_run(w, U0, nlive, *o));
}

extern "C" int mcalf_nested_advance(mcalf_ctx* ctx, int32_t max_rounds, mcalf_nested_state_t* out) {
    constexpr char name[] = "mcalf_nested_advance";
    if (max_rounds < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: max_rounds must be >= 0, got %d", name, max_rounds);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    mcalf_ctx* w = holder(ctx);
    NsRun& s = w->nsrun;
    if (s.phase == NsRun::kClosed) return set_err(ctx, MCALF_ERR_INVALID, "%s: no run is open (mcalf_nested_open)", name);
    if (s.phase == NsRun::kFinished) return set_err(ctx, MCALF_ERR_INVALID, "%s: the run is finished (mcalf_nested_finish): it only reads and closes", name);
    const int rc = lift(ctx, w, advance_run(w, max_rounds));
    if (out) *out = {s.nlive, s.ndead, s.rounds, s.nevals, s.unfinished, s.rows_launched, s.ev.logX, s.ev.logZ, s.max_key, s.reason, 0};
    return rc;
}

extern "C" int mcalf_nested_finish(mcalf_ctx* ctx, double* logZ, double* logZ_err, double* H) {
    constexpr char name[] = "mcalf_nested_finish";
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    mcalf_ctx* w = holder(ctx);
    NsRun& s = w->nsrun;
    if (s.phase == NsRun::kClosed) return set_err(ctx, MCALF_ERR_INVALID, "%s: no run is open (mcalf_nested_open)", name);
    if (s.phase == NsRun::kFinished) return set_err(ctx, MCALF_ERR_INVALID, "%s: the run is finished already", name);
    const int rc = lift(ctx, w, finish_run(w));
    if (rc) return rc;
    if (logZ) *logZ = s.logZ;
    if (logZ_err) *logZ_err = std::sqrt(std::max(s.H, 0.0) / (double)s.nlive);
    if (H) *H = s.H;
    return MCALF_OK;
}

extern "C" int mcalf_nested_read(mcalf_ctx* ctx, int64_t first, int64_t count, double* cube, double* theta, double* logL, double* logw) {
    constexpr char name[] = "mcalf_nested_read";
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    mcalf_ctx* w = holder(ctx);
    NsRun& s = w->nsrun;
    if (s.phase == NsRun::kClosed) return set_err(ctx, MCALF_ERR_INVALID, "%s: no run is open (mcalf_nested_open)", name);
    if (first < 0 || count < 0 || first > s.ndead || count > s.ndead - first)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: rows [%lld, %lld + %lld) are outside the %lld dead rows", name, (long long)first, (long long)first,
                       (long long)count, (long long)s.ndead);
    if (logw && s.phase != NsRun::kFinished) return set_err(ctx, MCALF_ERR_INVALID, "%s: logw exists only after mcalf_nested_finish", name);
    return lift(ctx, w, read_run(w, first, count, cube, theta, logL, logw));
}

extern "C" int mcalf_nested_last_round(mcalf_ctx* ctx, int32_t* dying, int32_t* pick, double* D, double* lmin) {
    constexpr char name[] = "mcalf_nested_last_round";
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    mcalf_ctx* w = holder(ctx);
    if (w->nsrun.phase == NsRun::kClosed) return set_err(ctx, MCALF_ERR_INVALID, "%s: no run is open (mcalf_nested_open)", name);
    if (!w->nsrun.have_last) return set_err(ctx, MCALF_ERR_INVALID, "%s: the run has not selected a round yet", name);
    return lift(ctx, w, last_round(w, dying, pick, D, lmin));
}

extern "C" int mcalf_nested_close(mcalf_ctx* ctx) {
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_nested_close: ctx is NULL");
    NsRun& s = holder(ctx)->nsrun;
    s.phase = NsRun::kClosed;
    s.have_last = false; s.timed = false; s.timing = false;
    s.logw.clear(); s.host_l.clear();
    return MCALF_OK;
}

extern "C" int mcalf_nested_footprint(const mcalf_ctx* ctx, int64_t* device_bytes) {
    if (!ctx || !device_bytes) return set_err(nullptr, MCALF_ERR_INVALID, "mcalf_nested_footprint: %s is NULL", !ctx ? "ctx" : "device_bytes");
    *device_bytes = (int64_t)holder(const_cast<mcalf_ctx*>(ctx))->nsrun.device_bytes();
    return MCALF_OK;
}

extern "C" int mcalf_nested_set_timing(mcalf_ctx* ctx, int32_t on) {
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_nested_set_timing: ctx is NULL");
    if (on != 0 && on != 1) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_nested_set_timing: on must be 0 or 1, got %d", on);
    holder(ctx)->nsrun.timing = on != 0;
    return MCALF_OK;
}

extern "C" int mcalf_nested_last_times(mcalf_ctx* ctx, double* ms) {
    constexpr char name[] = "mcalf_nested_last_times";
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ms) return set_err(ctx, MCALF_ERR_INVALID, "%s: ms is NULL", name);
    const NsRun& s = holder(ctx)->nsrun;
    if (s.phase == NsRun::kClosed) return set_err(ctx, MCALF_ERR_INVALID, "%s: no run is open (mcalf_nested_open)", name);
    if (!s.timed) return set_err(ctx, MCALF_ERR_INVALID, "%s: the last round was not timed (mcalf_nested_set_timing)", name);
    for (int i = 0; i < 7; ++i) ms[i] = s.last_ms[i];
    return MCALF_OK;
}
