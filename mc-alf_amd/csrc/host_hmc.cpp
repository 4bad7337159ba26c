// Host side of the Hamiltonian Monte Carlo kernels (hmc_kernels.hip): mcalf_hmc_batch and its _device form -- n independent
// walkers in the unit cube, each making trajectories of nleap leapfrog steps.  A driver over the gradient launch (host_grad.cpp:
// theta_logl_grad, exactly what mcalf_loglike_grad_batch_device issues) -- no Voigt code of its own.  A leapfrog step is one
// kernel of hmc_kernels.hip and one gradient launch over the n theta rows that kernel wrote; an iteration is the draw kernel,
// nleap launches with a step kernel between two of them, and the decide kernel, which also fills the chain slot.  Nothing is read
// back during a call: the loop is issued in one go.  The call's host arrays, scale and wid, reach the device in the argument
// blocks of put kernels, in stream order.
#include <cmath>

#include "hmc_args.h"
#include "host_ctx.h"

static_assert(sizeof(mcalf_hmc_opts) == 48, "mcalf_hmc_opts is 48 bytes");
static_assert(sizeof(HmcPutArgs) <= 4096 && kHmcPut % kHmcWave == 0, "a put kernel's argument block fits the 4 KB of kernel arguments; whole waves");

namespace {

constexpr int64_t kHmcMaxChainBytes = 4LL << 30;      // largest chain (CU and CL together) a call may keep on the device: the ensemble's

// The arrays of a call; scale and wid are host arrays in both entries.
struct HmcRows {
    const double* U0; const double* scale; const uint64_t* wid;
    double *U, *theta, *logL; int32_t *status, *naccept, *ndead;
    double *CU, *CL;
};

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.
int hmc_check(mcalf_ctx* ctx, const char* name, const HmcRows& r, int64_t n, const mcalf_hmc_opts* o) {
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (n < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 0, got %lld", name, (long long)n);
    if (n > 0 && !r.U0) return set_err(ctx, MCALF_ERR_INVALID, "%s: U0 is NULL", name);
    if (n > 0 && !r.scale) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale is NULL", name);
    if (n > 0 && !r.U) return set_err(ctx, MCALF_ERR_INVALID, "%s: U is NULL", name);
    if (n > 0 && !r.logL) return set_err(ctx, MCALF_ERR_INVALID, "%s: logL is NULL", name);
    if (n > 0 && !r.status) return set_err(ctx, MCALF_ERR_INVALID, "%s: status is NULL", name);
    if (n > 0 && !r.naccept) return set_err(ctx, MCALF_ERR_INVALID, "%s: naccept is NULL", name);
    if (n > 0 && !r.ndead) return set_err(ctx, MCALF_ERR_INVALID, "%s: ndead is NULL", name);
    if (o->nsteps < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nsteps must be >= 0, got %d", name, o->nsteps);
    if (o->thin < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: thin must be >= 1, got %d", name, o->thin);
    if (o->nleap < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: nleap must be >= 1, got %d", name, o->nleap);
    if (!std::isfinite(o->eps) || !(o->eps > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: eps must be finite and > 0, got %g", name, o->eps);
    if (!(o->jitter >= 0.0 && o->jitter < 1.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: jitter must be in [0, 1), got %g", name, o->jitter);
    if (n > 0x7fff0000LL) return set_err(ctx, MCALF_ERR_RANGE, "%s: nwalkers %lld too large", name, (long long)n);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    for (int k = 0; n > 0 && k < ctx->ndim; ++k)
        if (!std::isfinite(r.scale[k]) || r.scale[k] < 0.0)
            return set_err(ctx, MCALF_ERR_INVALID, "%s: scale[%d] must be finite and >= 0 (0: the coordinate is frozen), got %g", name, k, r.scale[k]);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the walkers move in its unit cube)", name);
    const int64_t per = n * ((r.CU ? (int64_t)ctx->ndim : 0) + (r.CL ? 1 : 0)) * (int64_t)sizeof(double), nkeep = o->nsteps / o->thin;
    if (per > 0 && nkeep > kHmcMaxChainBytes / per)
        return set_err(ctx, MCALF_ERR_RANGE, "%s: a chain of nkeep %lld slots of %lld walkers x %d coordinates exceeds the %lld bytes one call may keep "
                       "on the device; the largest nkeep for this ensemble is %lld (raise thin)", name, (long long)nkeep, (long long)n, ctx->ndim,
                       (long long)kHmcMaxChainBytes, (long long)(kHmcMaxChainBytes / per));
    return MCALF_OK;
}

// What a failed launch of a kernel of hmc_kernels.hip is reported as.
constexpr char kHmcLaunch[] = "hipLaunchKernel(hmc_kernel_ptr(k), dim3(grid), dim3(kHmcWave), args, 0, stream)";

// `count` 64-bit words of the host array `src` into the device array `dst`, kHmcPut at a time, in stream order.
int put_words(mcalf_ctx* ctx, uint64_t* dst, const void* src, size_t count, hipStream_t stream) {
    HmcPutArgs p;
    for (size_t at = 0; at < count; at += kHmcPut) {
        p.dst = dst + at;
        p.count = (int)std::min<size_t>(kHmcPut, count - at);
        memcpy(p.v, static_cast<const char*>(src) + at * sizeof(uint64_t), (size_t)p.count * sizeof(uint64_t));
        const int rc = launch_block(ctx, hmc_kernel_ptr(kHmcPutWords), p, dim3(1), dim3(kHmcPut), stream, kHmcLaunch);
        if (rc) return rc;
    }
    return MCALF_OK;
}

// The call over `n` device rows on `stream`: issued in one go, nothing is read back.
int run_hmc(mcalf_ctx* ctx, const HmcRows& r, int64_t n, const mcalf_hmc_opts& o, hipStream_t stream) {
    if (n <= 0) return MCALF_OK;
    const size_t nb = (size_t)n, ndim = (size_t)ctx->ndim, cells = nb * ndim;
    DevBuf<double>* hb = ctx->hmb;
    int rc;
    for (int b : {mcalf_ctx::kHmG, mcalf_ctx::kHmR, mcalf_ctx::kHmY, mcalf_ctx::kHmTheta, mcalf_ctx::kHmGY})
        if ((rc = grow(ctx, hb[b], cells))) return rc;
    if ((rc = grow(ctx, hb[mcalf_ctx::kHmLY], nb)) || (rc = grow(ctx, hb[mcalf_ctx::kHmAux], nb * kHmcAux)) ||
        (rc = grow(ctx, hb[mcalf_ctx::kHmScale], ndim)) || (rc = grow(ctx, ctx->hmc_dead, nb)) || (r.wid && (rc = grow(ctx, ctx->hmc_wid, nb))))
        return rc;
    static_assert(sizeof(double) == sizeof(uint64_t), "scale travels as 64-bit words");
    if ((rc = put_words(ctx, reinterpret_cast<uint64_t*>(hb[mcalf_ctx::kHmScale].p), r.scale, ndim, stream)) ||
        (r.wid && (rc = put_words(ctx, ctx->hmc_wid, r.wid, nb, stream))))
        return rc;
    HmcArgs a = {};
    a.U0 = r.U0; a.U = r.U; a.L = r.logL; a.status = r.status; a.naccept = r.naccept; a.ndead = r.ndead;
    a.G = hb[mcalf_ctx::kHmG]; a.R = hb[mcalf_ctx::kHmR]; a.Y = hb[mcalf_ctx::kHmY]; a.TH = hb[mcalf_ctx::kHmTheta];
    a.LY = hb[mcalf_ctx::kHmLY]; a.GY = hb[mcalf_ctx::kHmGY]; a.aux = hb[mcalf_ctx::kHmAux]; a.dead = ctx->hmc_dead;
    a.scale = hb[mcalf_ctx::kHmScale]; a.wid = r.wid ? ctx->hmc_wid.p : nullptr;
    a.seed = o.seed; a.eps = o.eps; a.jitter = o.jitter; a.n = (int)n; a.ndim = ctx->ndim;
    a.slot = ctx->startind; a.prior_int = ctx->prior_int;
    a.prior = prior_dev(ctx);
    const dim3 grid((unsigned)n), wave(kHmcWave);
    // the start: theta(U0), its logL straight into the caller's rows and its gradient, then the start kernel
    if ((rc = cube_to_theta(ctx, r.U0, a.TH, n, stream)) || (rc = theta_logl_grad(ctx, a.TH, a.L, hb[mcalf_ctx::kHmGY], n, stream)) ||
        (rc = launch_block(ctx, hmc_kernel_ptr(kHmcStart), a, grid, wave, stream, kHmcLaunch)))
        return rc;
    for (int i = 0; i < o.nsteps; ++i) {
        const bool keep = (i + 1) % o.thin == 0;
        const size_t slot = keep ? (size_t)((i + 1) / o.thin - 1) : 0;
        a.iter = o.first_iter + (uint64_t)i;
        a.CU = keep && r.CU ? r.CU + slot * cells : nullptr;
        a.CL = keep && r.CL ? r.CL + slot * nb : nullptr;
        if ((rc = launch_block(ctx, hmc_kernel_ptr(kHmcDraw), a, grid, wave, stream, kHmcLaunch))) return rc;
        for (int j = 0; j < o.nleap; ++j) {
            if ((rc = theta_logl_grad(ctx, a.TH, hb[mcalf_ctx::kHmLY], hb[mcalf_ctx::kHmGY], n, stream)) ||
                (rc = launch_block(ctx, hmc_kernel_ptr(j + 1 < o.nleap ? kHmcStep : kHmcDecide), a, grid, wave, stream, kHmcLaunch)))
                return rc;
        }
    }
    if (r.theta) return cube_to_theta(ctx, r.U, r.theta, n, stream);      // the transformed rows of the walkers
    return MCALF_OK;
}

// The host entry's call: the options, the host arrays, and the chain (the CU slots, then the CL slots), which lives as long as
// the call.
struct HmcCall { const char* name; const mcalf_hmc_opts* o; const double* scale; const uint64_t* wid; int64_t n; size_t nCU, nCL; DevBuf<double> chain; };
enum HmcCol { kColU0, kColU, kColTheta, kColL, kColStatus, kColNaccept, kColNdead, kColCU, kColCL, kHmcCols };

// The host entry's device driver (host_staged.cpp: run_staged) over the n rows; columns in the order of HmcCol, the chain's two
// its own.
int hmc_body(mcalf_ctx* ctx, void** dev, int64_t, hipStream_t stream, void* arg) {
    HmcCall* c = static_cast<HmcCall*>(arg);
    if (c->nCU + c->nCL > 0 && hipMalloc((void**)&c->chain.p, (c->nCU + c->nCL) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        c->chain.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "%s: no device memory for the chain of %zu slots (%.1f MB); raise thin", c->name,
                       (size_t)(c->o->nsteps / c->o->thin), (double)(c->nCU + c->nCL) * 8e-6);
    }
    dev[kColCU] = c->nCU ? c->chain.p : nullptr;
    dev[kColCL] = c->nCL ? c->chain.p + c->nCU : nullptr;
    const HmcRows d = {(const double*)dev[kColU0], c->scale, c->wid, (double*)dev[kColU], (double*)dev[kColTheta], (double*)dev[kColL],
                       (int32_t*)dev[kColStatus], (int32_t*)dev[kColNaccept], (int32_t*)dev[kColNdead], (double*)dev[kColCU], (double*)dev[kColCL]};
    const int rc = run_hmc(ctx, d, c->n, *c->o, stream);
    if (rc) (void)hipStreamSynchronize(stream);           // (the chain is freed behind the stream)
    return rc;
}

// All on one device: a multi-device context's first (see the header for what cutting the walkers would take).
int hmc_host(mcalf_ctx* ctx, const char* name, const HmcRows& r, int64_t n, const mcalf_hmc_opts& o) {
    const size_t d = sizeof(double), i = sizeof(int32_t), ndim = (size_t)ctx->ndim, nkeep = (size_t)(o.nsteps / o.thin);
    HmcCall call = {name, &o, r.scale, r.wid, n, r.CU ? nkeep * (size_t)n * ndim : 0, r.CL ? nkeep * (size_t)n : 0, {}};   // (the chain is released when the call returns)
    StagePlan plan = {{stage_in(r.U0, d, ndim), stage_out(r.U, d, ndim), stage_out(r.theta, d, ndim), stage_out(r.logL, d, 1), stage_out(r.status, i, 1),
                       stage_out(r.naccept, i, 1), stage_out(r.ndead, i, 1),
                       stage_out(r.CU, d, call.nCU, false, true), stage_out(r.CL, d, call.nCL, false, true)},
                      kHmcCols, n, kStageFirstDevice, kColU0, kColU, hmc_body, &call};
    plan.cols[kColCU].present = call.nCU > 0;             // (a call that keeps no slot has no chain)
    plan.cols[kColCL].present = call.nCL > 0;
    return run_staged(ctx, plan);
}

}  // namespace

extern "C" int mcalf_hmc_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const double* scale, const uint64_t* wid, const mcalf_hmc_opts* opts,
                               double* U, double* theta, double* logL, int32_t* status, int32_t* naccept, int32_t* ndead, double* CU, double* CL) {
    const HmcRows r = {U0, scale, wid, U, theta, logL, status, naccept, ndead, CU, CL};
    const int rc = hmc_check(ctx, "mcalf_hmc_batch", r, nwalkers, opts);
    if (rc) return rc;
    if (nwalkers == 0) return MCALF_OK;
    return hmc_host(ctx, "mcalf_hmc_batch", r, nwalkers, *opts);
}

extern "C" int mcalf_hmc_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const double* scale, const uint64_t* wid,
                                      const mcalf_hmc_opts* opts, double* dU, double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept,
                                      int32_t* dndead, double* dCU, double* dCL, void* stream) {
    const HmcRows r = {dU0, scale, wid, dU, dtheta, dlogL, dstatus, dnaccept, dndead, dCU, dCL};
    const int rc = hmc_check(ctx, "mcalf_hmc_batch_device", r, nwalkers, opts);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_hmc_batch_device");
    if (nwalkers == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_hmc(ctx, r, nwalkers, *opts, (hipStream_t)stream);
}
