// Host side of the nested-sampling kernels (ns_kernels.hip): the replacement primitive mcalf_slice_replace_batch -- a batch of
// chains in the unit cube moved by slice sampling under a hard likelihood constraint, in lock step.  A driver over the cube
// logL launch (host_launch.cpp: launch() with from_cube) -- no Voigt code of its own.  One step is the step kernel (decide on
// the last trial, propose the next) and one logL launch over the trial rows: the set-up kernel and the fused kernel, as
// mcalf_loglike_cube_batch_device issues them.  With mcalf_set_slice_compact on, the host entry's launch runs over the rows that
// proposed a trial only (pack and gather kernels in between: compact_steps).  mcalf_slice_last_stats says what a call launched.
#include <cmath>

#include "ns_args.h"
#include "host_ctx.h"

namespace {

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.  host_d: D is a host array
// whose entries are read here.
int ns_check(mcalf_ctx* ctx, const char* name, const NsRows& r, int64_t batch, const mcalf_slice_opts* o, bool host_d) {
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !r.U0) return set_err(ctx, MCALF_ERR_INVALID, "%s: U0 is NULL", name);
    if (batch > 0 && !r.Lmin) return set_err(ctx, MCALF_ERR_INVALID, "%s: Lmin is NULL", name);
    if (batch > 0 && !r.D) return set_err(ctx, MCALF_ERR_INVALID, "%s: D is NULL", name);
    if (batch > 0 && !r.sid) return set_err(ctx, MCALF_ERR_INVALID, "%s: sid is NULL", name);
    if (batch > 0 && !r.U) return set_err(ctx, MCALF_ERR_INVALID, "%s: U is NULL", name);
    if (batch > 0 && !r.logL) return set_err(ctx, MCALF_ERR_INVALID, "%s: logL is NULL", name);
    if (batch > 0 && !r.status) return set_err(ctx, MCALF_ERR_INVALID, "%s: status is NULL", name);
    if (batch > 0 && !r.nevals) return set_err(ctx, MCALF_ERR_INVALID, "%s: nevals is NULL", name);
    if (batch > 0 && !r.moves) return set_err(ctx, MCALF_ERR_INVALID, "%s: moves is NULL", name);
    if (o->nmoves < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nmoves must be >= 0, got %d", name, o->nmoves);
    if (o->max_steps < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: max_steps must be >= 0, got %d", name, o->max_steps);
    if (o->ndirs < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: ndirs must be >= 1, got %d", name, o->ndirs);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the chains move in its unit cube)", name);
    if (host_d && batch > 0)
        for (size_t i = 0, n = (size_t)o->ndirs * (size_t)ctx->ndim; i < n; ++i)
            if (!std::isfinite(r.D[i]))
                return set_err(ctx, MCALF_ERR_INVALID, "%s: D has a non-finite entry (row %zu, coordinate %zu: %g)", name, i / ctx->ndim, i % ctx->ndim, r.D[i]);
    return MCALF_OK;
}

// What a failed launch of a kernel of ns_kernels.hip is reported as.
constexpr char kNsLaunch[] = "hipLaunchKernel(ns_kernel_ptr(k), dim3(grid), dim3(block), args, 0, stream)";

// The lock steps of a call that packs its trial rows (mcalf_set_slice_compact; host entry only).  Live rows only ever finish, so
// the count of rows that proposed in step it - 1 bounds the count of step it: the launch of step it is sized by it, and the host
// reads the count of step it behind an event while the device is already in that step's logL launch -- the device never waits
// for the host.  The slots past the count hold the trial row of row 0 and are never read.  *open_trial: the last trial has been
// evaluated and not yet decided on.
int compact_steps(mcalf_ctx* ctx, NsArgs& a, const mcalf_slice_opts& o, hipStream_t stream, bool* open_trial) {
    mcalf_slice_stats_t& st = ctx->ns_stats;
    int rc;
    int64_t n = a.nrows;                                // count(0): every row may propose in step 1
    for (int it = 1; it <= o.max_steps && o.nmoves > 0; ++it) {
        a.it = it; a.decide = *open_trial ? 1 : 0; a.propose = 1;
        if ((rc = launch_block(ctx, ns_kernel_ptr(kNsStep), a, dim3((unsigned)a.nrows), dim3(kNsWave), stream, kNsLaunch)) ||
            (rc = launch_block(ctx, ns_kernel_ptr(kNsPack), a, dim3(1), dim3(kNsPackBlock), stream, kNsLaunch)))
            return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_ns_live, a.live, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_ns, stream));
        if ((rc = launch_block(ctx, ns_kernel_ptr(kNsGather), a, dim3((unsigned)n), dim3(kNsWave), stream, kNsLaunch)) ||
            (rc = cube_logl(ctx, a.Yc, a.LY, n, stream)))
            return rc;
        *open_trial = true;
        st.steps += 1; st.rows_launched += n;
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_ns));
        const int64_t c = *ctx->h_ns_live;
        st.trials += c;
        if (c == 0) { *open_trial = false; break; }     // (no row proposed: there is nothing left to decide)
        n = c;
    }
    return MCALF_OK;
}

// The call over `batch` device rows on `stream`.  poll: after every step the host reads the counter of rows that proposed a
// trial (4 bytes, through a page-locked word) and leaves the loop at 0 -- finished rows are carried, so the rows' bits are those
// of the unconditional max_steps steps the device entry runs.  A polling call of a context with ns_compact set packs its trial
// rows (compact_steps); the rows' bits are the same again.  (Declared in host_ctx.h: host_nsrun.cpp's rounds call it too.)
}  // namespace

int run_ns(mcalf_ctx* ctx, const NsRows& r, int64_t batch, const mcalf_slice_opts& o, hipStream_t stream, bool poll) {
    if (batch <= 0) return MCALF_OK;
    if (batch > 0x7fff0000LL) return set_err(ctx, MCALF_ERR_RANGE, "batch %lld too large", (long long)batch);
    const size_t nb = (size_t)batch, ndim = (size_t)ctx->ndim;
    const bool compact = poll && ctx->ns_compact;
    int rc;
    if ((rc = grow(ctx, ctx->nb[mcalf_ctx::kNbY], nb * ndim)) || (rc = grow(ctx, ctx->nb[mcalf_ctx::kNbLY], nb)) ||
        (rc = grow(ctx, ctx->nb[mcalf_ctx::kNbBrk], nb * kNsBrk)) || (rc = grow(ctx, ctx->ns_dir, nb)) || (rc = grow(ctx, ctx->d_ns_live, 1)) ||
        (rc = grow(ctx, ctx->ns_pack, nb * kNsPackInts)) || (compact && (rc = grow(ctx, ctx->nb[mcalf_ctx::kNbYc], nb * ndim))))
        return rc;
    if (poll && !ctx->h_ns_live.p) HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_ns_live.p, sizeof(unsigned int), hipHostMallocDefault));
    if (compact && !ctx->ev_ns) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_ns, hipEventDisableTiming));
    mcalf_slice_stats_t& st = ctx->ns_stats;
    st = mcalf_slice_stats_t();
    st.batch = batch; st.rows_launched = batch; st.compact = compact ? 1 : 0;
    NsArgs a = {};
    a.U0 = r.U0; a.Lmin = r.Lmin; a.D = r.D; a.sid = r.sid; a.U = r.U; a.L = r.logL; a.status = r.status; a.nevals = r.nevals; a.moves = r.moves;
    a.Y = ctx->nb[mcalf_ctx::kNbY]; a.LY = ctx->nb[mcalf_ctx::kNbLY]; a.brk = ctx->nb[mcalf_ctx::kNbBrk]; a.dir = ctx->ns_dir; a.live = ctx->d_ns_live;
    a.stamp = ctx->ns_pack;
    a.prior = prior_dev(ctx);
    a.seed = o.seed; a.nrows = (int)batch; a.ndim = ctx->ndim; a.ndirs = o.ndirs; a.nmoves = o.nmoves;
    const dim3 rows((unsigned)batch), wave(kNsWave);
    if ((rc = launch_block(ctx, ns_kernel_ptr(kNsStart), a, rows, wave, stream, kNsLaunch)) || (rc = cube_logl(ctx, a.Y, a.LY, batch, stream)) ||
        (rc = launch_block(ctx, ns_kernel_ptr(kNsStarted), a, rows, wave, stream, kNsLaunch)))
        return rc;
    bool open_trial = false;                            // the last trial has been evaluated and not yet decided on
    if (compact) {                                      // (from here on LY holds the logL of the packed rows, by slot)
        a.slot = ctx->ns_pack + nb; a.idx = ctx->ns_pack + 2 * nb; a.Yc = ctx->nb[mcalf_ctx::kNbYc];
        if ((rc = compact_steps(ctx, a, o, stream, &open_trial))) return rc;
    } else {
        for (int it = 1; it <= o.max_steps && o.nmoves > 0; ++it) {
            if (poll) HIP_TRY(ctx, hipMemsetAsync(a.live, 0, sizeof(unsigned int), stream));
            a.it = it; a.decide = open_trial ? 1 : 0; a.propose = 1;
            if ((rc = launch_block(ctx, ns_kernel_ptr(kNsStep), a, rows, wave, stream, kNsLaunch))) return rc;
            if (poll) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_ns_live, a.live, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
            if ((rc = cube_logl(ctx, a.Y, a.LY, batch, stream))) return rc;
            open_trial = true;
            st.steps += 1; st.rows_launched += batch;
            if (poll) {
                HIP_TRY(ctx, hipStreamSynchronize(stream));
                st.trials += *ctx->h_ns_live;
                if (*ctx->h_ns_live == 0) { open_trial = false; break; }      // (no row proposed: there is nothing left to decide)
            }
        }
        if (!poll) st.trials = -1;                      // (the device entry never learns the counts)
    }
    if (open_trial) {
        a.it = o.max_steps + 1; a.decide = 1; a.propose = 0;
        if ((rc = launch_block(ctx, ns_kernel_ptr(kNsStep), a, rows, wave, stream, kNsLaunch))) return rc;
    }
    if (r.theta) return cube_to_theta(ctx, r.U, r.theta, batch, stream);      // the transformed rows of the points
    return MCALF_OK;
}

namespace {

// The host entry's device driver (host_staged.cpp: run_staged); columns in the order of NsCol.
enum NsCol { kColU0, kColLmin, kColD, kColSid, kColU, kColTheta, kColL, kColStatus, kColNevals, kColMoves, kNsCols };

int ns_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    const NsRows d = {(const double*)dev[kColU0], (const double*)dev[kColLmin], (const double*)dev[kColD], (const uint64_t*)dev[kColSid],
                      (double*)dev[kColU], (double*)dev[kColTheta], (double*)dev[kColL], (int32_t*)dev[kColStatus], (int32_t*)dev[kColNevals],
                      (int32_t*)dev[kColMoves]};
    return run_ns(ctx, d, rows, *static_cast<const mcalf_slice_opts*>(arg), stream, true);
}

int ns_host(mcalf_ctx* ctx, const NsRows& r, int64_t batch, const mcalf_slice_opts& o) {
    const size_t d = sizeof(double), i = sizeof(int32_t), ndim = (size_t)ctx->ndim;
    StagePlan plan = {{stage_in(r.U0, d, ndim), stage_in(r.Lmin, d, 1), stage_in(r.D, d, (size_t)o.ndirs * ndim, false), stage_in(r.sid, sizeof(uint64_t), 1),
                       stage_out(r.U, d, ndim), stage_out(r.theta, d, ndim), stage_out(r.logL, d, 1), stage_out(r.status, i, 1),
                       stage_out(r.nevals, i, 1), stage_out(r.moves, i, 1)},
                      kNsCols, batch, kStageCutRows, kColU0, kColU, ns_body, const_cast<mcalf_slice_opts*>(&o)};
    const int rc = run_staged(ctx, plan);
    if (is_multi(ctx)) {
        mcalf_slice_stats_t& st = ctx->ns_stats;          // the sum over the entries the call was cut over; the longest loop
        st = mcalf_slice_stats_t();
        st.compact = ctx->ns_compact;
        for (int k = 0; k < ctx->multi_last_active; ++k) {
            const mcalf_slice_stats_t& e = ctx->subs[k]->ns_stats;
            st.batch += e.batch; st.rows_launched += e.rows_launched; st.trials += e.trials;
            st.steps = std::max(st.steps, e.steps);
        }
    }
    return rc;
}

}  // namespace

extern "C" int mcalf_slice_replace_batch(mcalf_ctx* ctx, const double* U0, const double* Lmin, const double* D, const uint64_t* sid,
                                         int64_t batch, const mcalf_slice_opts* opts, double* U, double* theta, double* logL,
                                         int32_t* status, int32_t* nevals, int32_t* moves) {
    const NsRows r = {U0, Lmin, D, sid, U, theta, logL, status, nevals, moves};
    const int rc = ns_check(ctx, "mcalf_slice_replace_batch", r, batch, opts, true);
    if (rc) return rc;
    ctx->ns_stats = mcalf_slice_stats_t();
    if (batch == 0) return MCALF_OK;
    return ns_host(ctx, r, batch, *opts);
}

extern "C" int mcalf_slice_replace_batch_device(mcalf_ctx* ctx, const double* dU0, const double* dLmin, const double* dD, const uint64_t* dsid,
                                                int64_t batch, const mcalf_slice_opts* opts, double* dU, double* dtheta, double* dlogL,
                                                int32_t* dstatus, int32_t* dnevals, int32_t* dmoves, void* stream) {
    const NsRows r = {dU0, dLmin, dD, dsid, dU, dtheta, dlogL, dstatus, dnevals, dmoves};
    const int rc = ns_check(ctx, "mcalf_slice_replace_batch_device", r, batch, opts, false);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_slice_replace_batch_device");
    ctx->ns_stats = mcalf_slice_stats_t();
    if (batch == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_ns(ctx, r, batch, *opts, (hipStream_t)stream, false);
}

extern "C" int mcalf_set_slice_compact(mcalf_ctx* ctx, int32_t on) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "mcalf_set_slice_compact: ctx is NULL");
    if (on != 0 && on != 1) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_set_slice_compact: on must be 0 or 1, got %d", on);
    ctx->ns_compact = on;
    for (mcalf_ctx* sub : ctx->subs) sub->ns_compact = on;
    return MCALF_OK;
}

extern "C" int mcalf_slice_last_stats(const mcalf_ctx* ctx, mcalf_slice_stats_t* out) {
    if (!ctx || !out) return set_err(nullptr, MCALF_ERR_INVALID, "mcalf_slice_last_stats: %s is NULL", !ctx ? "ctx" : "out");
    *out = ctx->ns_stats;
    return MCALF_OK;
}
