// Host side of the chain-diagnostics kernels (chain_kernels.h): mcalf_chain_stats, mcalf_ensemble_converge and their _device
// forms.  One driver (run_stats) issues the statistics of a chain prefix: the pass over the walkers' series, then the same lag
// pass over the one series of ensemble means.  run_converge puts it behind blocks of the ensemble sampler's own driver
// (host_ens.cpp: run_ens) and reads tau and the flags back after every check -- the one place the sampler family waits.
// Compiled as part of host_ens.cpp's translation unit (its last line includes this file): the run to convergence is built from
// that file's own EnsRows, ens_check, one_temperature and run_ens, which stay internal to it.  NOT a stand-alone header: it
// defines extern "C" entries and uses host_ens.cpp's anonymous namespace; nothing else may include it.
#pragma once
#include "chain_args.h"

static_assert(sizeof(mcalf_chain_opts) == 16, "mcalf_chain_opts is 16 bytes");
static_assert(sizeof(mcalf_converge_opts) == 32, "mcalf_converge_opts is 32 bytes");

namespace {

constexpr int64_t kChainMaxPartBytes = 1LL << 30;     // largest workspace of walker-block partial ACFs a call may take
constexpr int64_t kChainMaxElems = 1LL << 59;         // nkeep x nwalkers x ndim doubles must stay far inside size_t

int64_t chain_blocks(int64_t n) { return (n + kChainWalkerBlock - 1) / kChainWalkerBlock; }
int64_t chain_lag(int64_t T, const mcalf_chain_opts& o) { return o.max_lag == 0 ? T - 1 : o.max_lag; }
// doubles of one pass's workspace: the 9 per-walker arrays, the pool, the partial ACFs and the ACF
size_t pass_elems(int64_t n, int d, int64_t L) {
    return (size_t)n * d * 9 + (size_t)d * kChainPool + (size_t)chain_blocks(n) * d * (size_t)(L + 1) + (size_t)d * (size_t)(L + 1);
}
// ... of a call: the walkers' pass, the mean series [T][d], the mean series' pass
size_t stats_elems(int64_t T, int64_t n, int d, int64_t L) { return pass_elems(n, d, L) + (size_t)T * d + pass_elems(1, d, L); }

// Everything that is wrong with a statistics call before any device work; `name` is the entry that reports it.
int chain_check(mcalf_ctx* ctx, const char* name, const double* X, int64_t T, int64_t n, int32_t d, const mcalf_chain_opts* o,
                const double* stats, const int32_t* info) {
    if (!X) return set_err(ctx, MCALF_ERR_INVALID, "%s: X is NULL", name);
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (!stats) return set_err(ctx, MCALF_ERR_INVALID, "%s: stats is NULL", name);
    if (!info) return set_err(ctx, MCALF_ERR_INVALID, "%s: info is NULL", name);
    if (T < 4) return set_err(ctx, MCALF_ERR_INVALID, "%s: nkeep must be >= 4 (split R-hat needs halves of at least 2), got %lld", name, (long long)T);
    if (n < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 1, got %lld", name, (long long)n);
    if (d < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: ndim must be >= 1, got %d", name, d);
    if (!std::isfinite(o->c) || !(o->c > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: c must be finite and > 0, got %g", name, o->c);
    if (o->max_lag < 0 || o->max_lag > T - 1)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: max_lag must be 0 (nkeep - 1) or in [1, nkeep - 1 = %lld], got %lld", name, (long long)(T - 1), (long long)o->max_lag);
    if (T > kChainMaxElems / n || T * n > kChainMaxElems / d || T > 0x7fffffffLL)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: nkeep x nwalkers x ndim = %lld x %lld x %d overflows", name, (long long)T, (long long)n, d);
    const int64_t L = chain_lag(T, *o), per_lag = chain_blocks(n) * d * (int64_t)sizeof(double);
    if (chain_blocks(n) > 0x7fffffffLL || (d + kChainKT - 1) / kChainKT > 65535 || L / kChainLT + 1 > 65535)
        return set_err(ctx, MCALF_ERR_RANGE, "%s: nwalkers %lld, ndim %d or the lag %lld exceeds the lag kernel's grid", name, (long long)n, d, (long long)L);
    if (L + 1 > kChainMaxPartBytes / per_lag)
        return set_err(ctx, MCALF_ERR_RANGE, "%s: the partial sums of %lld lags of %lld walker blocks x %d coordinates exceed the %lld bytes a call "
                       "may take; the largest max_lag that fits is %lld", name, (long long)(L + 1), (long long)chain_blocks(n), d,
                       (long long)kChainMaxPartBytes, (long long)(kChainMaxPartBytes / per_lag - 1));
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    return MCALF_OK;
}

// The workspace of one pass, carved from `p`; returns the first double behind it.
double* carve_pass(ChainArgs& a, double* p) {
    const size_t nd = (size_t)a.n * a.d, L1 = (size_t)(a.L + 1);
    a.sum = p; a.mu = p + nd; a.c0 = p + 2 * nd; a.sq = p + 3 * nd; a.hm = p + 4 * nd; a.hv = p + 6 * nd; a.kf = p + 8 * nd;
    p += 9 * nd;
    a.pool = p; p += (size_t)a.d * kChainPool;
    a.part = p; p += (size_t)a.nblocks * a.d * L1;
    a.rho = p; p += (size_t)a.d * L1;
    return p;
}

unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// The kernels of one pass, in order.
int issue_pass(mcalf_ctx* ctx, const ChainArgs& a, hipStream_t stream) {
    const size_t nd = (size_t)a.n * a.d, L1 = (size_t)(a.L + 1);
    const dim3 per_series(blocks_of(nd, 256)), per_coord((unsigned)a.d);
    const dim3 lag_grid((unsigned)a.nblocks, (unsigned)(a.L / kChainLT + 1), (unsigned)((a.d + kChainKT - 1) / kChainKT));
    int rc;
    if ((rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainSums), a, per_series, dim3(256), stream)) ||
        (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainPoolMean), a, per_coord, dim3(64), stream)) ||
        (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainCentred), a, per_series, dim3(256), stream)) ||
        (!a.mean_series && (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainMeanSeries), a, dim3((unsigned)a.T), dim3(64), stream))) ||
        (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainPoolVar), a, per_coord, dim3(64), stream)) ||
        (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainLag), a, lag_grid, dim3(kChainBlock), stream)) ||
        (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainAcf), a, dim3(blocks_of((size_t)a.d * L1, 256)), dim3(256), stream)) ||
        (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainTau), a, dim3(blocks_of((size_t)a.d, 64)), dim3(64), stream)))
        return rc;
    return MCALF_OK;
}

// The statistics of the chain dX [T][n][d] on `stream`, device pointers: the workspace (grown once: a later call of the same or
// a smaller size allocates nothing), the walkers' pass, then the pass over the series of ensemble means.
int run_stats(mcalf_ctx* ctx, const double* dX, int64_t T, int64_t n, int d, const int32_t* dstatus, double c, int64_t L, double* dstats,
              int32_t* dinfo, double* dacf, hipStream_t stream) {
    if (L / kChainLT + 1 > 65535) return set_err(ctx, MCALF_ERR_RANGE, "chain statistics: the lag %lld exceeds the lag kernel's grid", (long long)L);
    int rc;
    if ((rc = grow(ctx, ctx->chain_ws, stats_elems(T, n, d, L)))) return rc;
    ChainArgs a = {};
    a.X = dX; a.status = dstatus; a.stats = dstats; a.info = dinfo; a.acf = dacf;
    a.T = T; a.n = n; a.L = L; a.d = d; a.nblocks = (int)chain_blocks(n); a.c = c;
    a.mser = carve_pass(a, ctx->chain_ws);
    if ((rc = issue_pass(ctx, a, stream))) return rc;
    ChainArgs m = a;                                      // the mean series as a chain of one walker
    m.X = a.mser; m.status = nullptr; m.acf = nullptr; m.n = 1; m.nblocks = 1; m.mean_series = 1;
    carve_pass(m, a.mser + (size_t)T * d);
    return issue_pass(ctx, m, stream);
}

struct StatsCall { int64_t T, n; int d; double c; int64_t L; };
enum StatsCol { kStX, kStStatus, kStStats, kStInfo, kStAcf, kStatsCols };

int stats_body(mcalf_ctx* ctx, void** dev, int64_t, hipStream_t stream, void* arg) {
    const StatsCall* s = static_cast<const StatsCall*>(arg);
    return run_stats(ctx, (const double*)dev[kStX], s->T, s->n, s->d, (const int32_t*)dev[kStStatus], s->c, s->L, (double*)dev[kStStats],
                     (int32_t*)dev[kStInfo], (double*)dev[kStAcf], stream);
}

// ---- the run to convergence ---------------------------------------------------------------------------------------------

int conv_check(mcalf_ctx* ctx, const char* name, const mcalf_converge_opts* cv, const double* CU, const int64_t* nkept, const int32_t* converged,
               const int32_t* nchecks, const double* tau_hist, const double* stats, const int32_t* info) {
    if (!cv) return set_err(ctx, MCALF_ERR_INVALID, "%s: conv is NULL", name);
    if (!nkept) return set_err(ctx, MCALF_ERR_INVALID, "%s: nkept is NULL", name);
    if (!converged) return set_err(ctx, MCALF_ERR_INVALID, "%s: converged is NULL", name);
    if (!nchecks) return set_err(ctx, MCALF_ERR_INVALID, "%s: nchecks is NULL", name);
    if (!tau_hist) return set_err(ctx, MCALF_ERR_INVALID, "%s: tau_hist is NULL", name);
    if (!stats) return set_err(ctx, MCALF_ERR_INVALID, "%s: stats is NULL", name);
    if (!info) return set_err(ctx, MCALF_ERR_INVALID, "%s: info is NULL", name);
    if (!CU) return set_err(ctx, MCALF_ERR_INVALID, "%s: CU is NULL (the statistics are the chain's)", name);
    if (cv->check_every < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: check_every must be >= 1, got %d", name, cv->check_every);
    if (!std::isfinite(cv->factor) || !(cv->factor > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: factor must be finite and > 0, got %g", name, cv->factor);
    if (!std::isfinite(cv->rtol) || cv->rtol < 0.0) return set_err(ctx, MCALF_ERR_INVALID, "%s: rtol must be finite and >= 0, got %g", name, cv->rtol);
    if (!std::isfinite(cv->c) || !(cv->c > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: c must be finite and > 0, got %g", name, cv->c);
    return MCALF_OK;
}

// The lag of a check over T kept steps.
int64_t check_lag(int64_t T, const mcalf_converge_opts& cv) {
    const double want = std::ceil(cv.c * (double)T / cv.factor) + 1.0;
    return want < (double)(T - 1) ? (int64_t)want : T - 1;
}

struct ConvOut { int64_t* nkept; int32_t *converged, *nchecks; double* tau_hist; };

// The run over `n` device rows on `stream`: blocks of run_ens, a check behind each, tau and the flags read back after it.
int run_converge(mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_ens_opts& eo, const mcalf_converge_opts& cv, double* dstats,
                 int32_t* dinfo, const ConvOut& out, hipStream_t stream) {
    const int d = ctx->ndim;
    const size_t nd = (size_t)n * d;
    const int64_t nkeep = eo.nsteps / eo.thin, total = nkeep * eo.thin;     // (iterations behind the last kept one are not made)
    *out.nkept = 0; *out.converged = 0; *out.nchecks = 0;
    int rc;
    if ((rc = grow(ctx, ctx->chain_u, nd)) || (rc = grow(ctx, ctx->chain_acc, (size_t)n))) return rc;
    if (nkeep >= 4 && (rc = grow(ctx, ctx->chain_ws, stats_elems(nkeep, n, d, check_lag(nkeep, cv))))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(r.naccept, 0, (size_t)n * sizeof(int32_t), stream));
    HIP_TRY(ctx, hipMemsetAsync(dstats, 0, (size_t)d * 6 * sizeof(double), stream));
    HIP_TRY(ctx, hipMemsetAsync(dinfo, 0, (size_t)d * 4 * sizeof(int32_t), stream));
    std::vector<double> hstats((size_t)d * 6), prev;
    std::vector<int32_t> hinfo((size_t)d * 4);
    const ChainAddArgs add = {r.naccept, ctx->chain_acc, n};
    int64_t done = 0, T = 0;                              // iterations made, kept steps so far
    const double* from = r.U0;
    bool stop = false;
    while (!stop) {
        const int64_t len = std::min<int64_t>((int64_t)cv.check_every * eo.thin, total - done);
        mcalf_ens_opts bo = eo;
        bo.nsteps = (int32_t)len; bo.first_iter = eo.first_iter + (uint64_t)done;
        const EnsRows br = {from, r.U, nullptr, r.logL, r.status, ctx->chain_acc, nullptr, r.CU + (size_t)T * nd, r.CL ? r.CL + (size_t)T * n : nullptr};
        if ((rc = run_ens(ctx, br, n, one_temperature(bo), kBetaOne, stream)) ||
            (rc = LAUNCH_BLOCK(ctx, chain_kernel_ptr(kChainAddInt), add, dim3(blocks_of((size_t)n, 256)), dim3(256), stream)))
            return rc;
        done += len; T += len / eo.thin;
        stop = done >= total;
        if (T >= 4 && len > 0) {
            if ((rc = run_stats(ctx, r.CU, T, n, d, r.status, cv.c, check_lag(T, cv), dstats, dinfo, nullptr, stream))) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(hstats.data(), dstats, hstats.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIP_TRY(ctx, hipMemcpyAsync(hinfo.data(), dinfo, hinfo.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(ctx, hipStreamSynchronize(stream));
            const int j = ++*out.nchecks;
            bool ok = j >= 2;
            for (int k = 0; k < d; ++k) {
                const double tau = hstats[(size_t)k * 6 + 2];
                out.tau_hist[(size_t)(j - 1) * d + k] = tau;
                if (hinfo[(size_t)k * 4 + 2] <= 0 || !ok) continue;          // a frozen coordinate; or the verdict is in
                ok = (hinfo[(size_t)k * 4 + 3] & 1) && (double)T >= cv.factor * tau && std::fabs(tau - prev[k]) <= cv.rtol * tau;
            }
            prev.assign(out.tau_hist + (size_t)(j - 1) * d, out.tau_hist + (size_t)j * d);
            if (ok) { *out.converged = 1; stop = true; }
        }
        if (!stop) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->chain_u, r.U, nd * sizeof(double), hipMemcpyDeviceToDevice, stream));
            from = ctx->chain_u;
        }
    }
    *out.nkept = T;
    if (r.theta) return cube_to_theta(ctx, r.U, r.theta, n, stream);
    return MCALF_OK;
}

// The host entry's call: the chain (the CU slots, then the CL slots) lives as long as the call; its first nkept slots go to the
// caller's arrays behind the run.
struct ConvCall {
    const mcalf_ens_opts* eo; const mcalf_converge_opts* cv; int64_t n; double *CU, *CL; ConvOut out; DevBuf<double> chain;
};
enum ConvCol { kCvU0, kCvU, kCvTheta, kCvL, kCvStatus, kCvNaccept, kCvStats, kCvInfo, kConvCols };

int conv_body(mcalf_ctx* ctx, void** dev, int64_t, hipStream_t stream, void* arg) {
    ConvCall* c = static_cast<ConvCall*>(arg);
    const size_t nd = (size_t)c->n * ctx->ndim, nkeep = (size_t)(c->eo->nsteps / c->eo->thin);
    const size_t nCU = nkeep * nd, nCL = c->CL ? nkeep * (size_t)c->n : 0;
    if (nCU + nCL > 0 && hipMalloc((void**)&c->chain.p, (nCU + nCL) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        c->chain.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "mcalf_ensemble_converge: no device memory for the chain of %zu slots (%.1f MB); raise thin", nkeep,
                       (double)(nCU + nCL) * 8e-6);
    }
    const EnsRows r = {(const double*)dev[kCvU0], (double*)dev[kCvU], (double*)dev[kCvTheta], (double*)dev[kCvL], (int32_t*)dev[kCvStatus],
                       (int32_t*)dev[kCvNaccept], nullptr, c->chain.p, nCL ? c->chain.p + nCU : nullptr};
    int rc = run_converge(ctx, r, c->n, *c->eo, *c->cv, (double*)dev[kCvStats], (int32_t*)dev[kCvInfo], c->out, stream);
    const size_t kept = (size_t)*c->out.nkept;
    if (!rc && kept > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(c->CU, r.CU, kept * nd * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (nCL) HIP_TRY(ctx, hipMemcpyAsync(c->CL, r.CL, kept * (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    if (rc) (void)hipStreamSynchronize(stream);           // (the chain is freed behind the stream)
    return rc;
}

}  // namespace

extern "C" int mcalf_chain_stats(mcalf_ctx* ctx, const double* X, int64_t nkeep, int64_t nwalkers, int32_t ndim, const int32_t* status,
                                 const mcalf_chain_opts* opts, double* stats, int32_t* info, double* acf) {
    const int rc = chain_check(ctx, "mcalf_chain_stats", X, nkeep, nwalkers, ndim, opts, stats, info);
    if (rc) return rc;
    StatsCall call = {nkeep, nwalkers, ndim, opts->c, chain_lag(nkeep, *opts)};
    const size_t dd = (size_t)ndim, L1 = (size_t)(call.L + 1);
    StagePlan plan = {{stage_in(X, sizeof(double), (size_t)nkeep * (size_t)nwalkers * dd, false), stage_in(status, sizeof(int32_t), (size_t)nwalkers, false),
                       stage_out(stats, sizeof(double), dd * 6, false), stage_out(info, sizeof(int32_t), dd * 4, false),
                       stage_out(acf, sizeof(double), dd * L1, false)},
                      kStatsCols, 1, kStageFirstDevice, kStX, kStStats, stats_body, &call};
    return run_staged(ctx, plan);
}

extern "C" int mcalf_chain_stats_device(mcalf_ctx* ctx, const double* dX, int64_t nkeep, int64_t nwalkers, int32_t ndim, const int32_t* dstatus,
                                        const mcalf_chain_opts* opts, double* dstats, int32_t* dinfo, double* dacf, void* stream) {
    const int rc = chain_check(ctx, "mcalf_chain_stats_device", dX, nkeep, nwalkers, ndim, opts, dstats, dinfo);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_chain_stats_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_stats(ctx, dX, nkeep, nwalkers, ndim, dstatus, opts->c, chain_lag(nkeep, *opts), dstats, dinfo, dacf, (hipStream_t)stream);
}

extern "C" int mcalf_ensemble_converge(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const mcalf_ens_opts* opts, const mcalf_converge_opts* conv,
                                       double* U, double* theta, double* logL, int32_t* status, int32_t* naccept, double* CU, double* CL,
                                       int64_t* nkept, int32_t* converged, int32_t* nchecks, double* tau_hist, double* stats, int32_t* info) {
    const char* name = "mcalf_ensemble_converge";
    int rc = conv_check(ctx, name, conv, CU, nkept, converged, nchecks, tau_hist, stats, info);
    if (rc) return rc;
    const EnsRows r = {U0, U, theta, logL, status, naccept, nullptr, CU, CL};
    const mcalf_pt_opts o = opts ? one_temperature(*opts) : mcalf_pt_opts();
    if (nwalkers == 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 4, got 0", name);
    if ((rc = ens_check(ctx, name, r, nwalkers, opts ? &o : nullptr, kBetaOne, false))) return rc;
    ConvCall call = {opts, conv, nwalkers, CU, CL, {nkept, converged, nchecks, tau_hist}, {}};     // (the chain is released when the call returns)
    const size_t d = sizeof(double), i = sizeof(int32_t), ndim = (size_t)ctx->ndim;
    StagePlan plan = {{stage_in(U0, d, ndim), stage_out(U, d, ndim), stage_out(theta, d, ndim), stage_out(logL, d, 1), stage_out(status, i, 1),
                       stage_out(naccept, i, 1), stage_out(stats, d, ndim * 6, false), stage_out(info, i, ndim * 4, false)},
                      kConvCols, nwalkers, kStageFirstDevice, kCvU0, kCvU, conv_body, &call};
    return run_staged(ctx, plan);
}

extern "C" int mcalf_ensemble_converge_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const mcalf_ens_opts* opts,
                                              const mcalf_converge_opts* conv, double* dU, double* dtheta, double* dlogL, int32_t* dstatus,
                                              int32_t* dnaccept, double* dCU, double* dCL, int64_t* nkept, int32_t* converged, int32_t* nchecks,
                                              double* tau_hist, double* dstats, int32_t* dinfo, void* stream) {
    const char* name = "mcalf_ensemble_converge_device";
    int rc = conv_check(ctx, name, conv, dCU, nkept, converged, nchecks, tau_hist, dstats, dinfo);
    if (rc) return rc;
    const EnsRows r = {dU0, dU, dtheta, dlogL, dstatus, dnaccept, nullptr, dCU, dCL};
    const mcalf_pt_opts o = opts ? one_temperature(*opts) : mcalf_pt_opts();
    if (nwalkers == 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 4, got 0", name);
    if ((rc = ens_check(ctx, name, r, nwalkers, opts ? &o : nullptr, kBetaOne, false))) return rc;
    MCALF_SINGLE_ONLY(ctx, name);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_converge(ctx, r, nwalkers, *opts, *conv, dstats, dinfo, {nkept, converged, nchecks, tau_hist}, (hipStream_t)stream);
}
