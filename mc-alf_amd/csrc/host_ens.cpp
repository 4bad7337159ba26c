// Host side of the ensemble-sampler kernels (ens_kernels.hip): mcalf_ensemble_batch and mcalf_ensemble_batch_device -- n walkers
// in the unit cube moved by the stretch or the DE move, half against half.  A driver over the cube logL launch (host_launch.cpp:
// launch() with from_cube) -- no Voigt code of its own.  A half-step is the propose kernel, one logL launch over the m trial
// rows (the set-up kernel and the fused kernel, as mcalf_loglike_cube_batch_device issues them) and the decide kernel, which also
// fills the chain slot of an iteration that is kept.  Nothing is read back during a call: the loop is issued in one go.
#include <cmath>

#include "ens_args.h"
#include "host_ctx.h"

static_assert(sizeof(mcalf_ens_opts) == 40, "mcalf_ens_opts is 40 bytes");
static_assert((int)MCALF_ENS_STRETCH == (int)kEnsStretch && (int)MCALF_ENS_DE == (int)kEnsDE, "the kernels' move numbers are the header's");

namespace {

constexpr int64_t kEnsMaxChainBytes = 4LL << 30;      // largest chain (CU and CL together) a call may keep on the device

struct EnsRows {
    const double* U0;
    double *U, *theta, *logL; int32_t *status, *naccept;
    double *CU, *CL;
};

// Bytes one chain slot takes on the device: the arrays the caller wants.
int64_t slot_bytes(const mcalf_ctx* ctx, const EnsRows& r, int64_t n) {
    return n * ((r.CU ? (int64_t)ctx->ndim : 0) + (r.CL ? 1 : 0)) * (int64_t)sizeof(double);
}

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.
int ens_check(mcalf_ctx* ctx, const char* name, const EnsRows& r, int64_t n, const mcalf_ens_opts* o) {
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (n < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 0, got %lld", name, (long long)n);
    if (n % 2 != 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be even (two halves move in turn), got %lld", name, (long long)n);
    if (n > 0 && n < 4) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 4 (the DE move takes two partners from a half), got %lld", name, (long long)n);
    if (n > 0 && !r.U0) return set_err(ctx, MCALF_ERR_INVALID, "%s: U0 is NULL", name);
    if (n > 0 && !r.U) return set_err(ctx, MCALF_ERR_INVALID, "%s: U is NULL", name);
    if (n > 0 && !r.logL) return set_err(ctx, MCALF_ERR_INVALID, "%s: logL is NULL", name);
    if (n > 0 && !r.status) return set_err(ctx, MCALF_ERR_INVALID, "%s: status is NULL", name);
    if (n > 0 && !r.naccept) return set_err(ctx, MCALF_ERR_INVALID, "%s: naccept is NULL", name);
    if (o->nsteps < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nsteps must be >= 0, got %d", name, o->nsteps);
    if (o->thin < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: thin must be >= 1, got %d", name, o->thin);
    if (o->move != MCALF_ENS_STRETCH && o->move != MCALF_ENS_DE)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: move must be MCALF_ENS_STRETCH (0) or MCALF_ENS_DE (1), got %d", name, o->move);
    if (!std::isfinite(o->scale)) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale must be finite, got %g", name, o->scale);
    if (o->move == MCALF_ENS_STRETCH && !(o->scale > 1.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale must be > 1 for the stretch move, got %g", name, o->scale);
    if (o->move == MCALF_ENS_DE && !(o->scale > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale must be > 0 for the DE move, got %g", name, o->scale);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the walkers move in its unit cube)", name);
    if (n > 0x7fff0000LL) return set_err(ctx, MCALF_ERR_RANGE, "%s: nwalkers %lld too large", name, (long long)n);
    const int64_t per = slot_bytes(ctx, r, n), nkeep = o->nsteps / o->thin;
    if (per > 0 && nkeep > kEnsMaxChainBytes / per)
        return set_err(ctx, MCALF_ERR_RANGE, "%s: a chain of nkeep %lld slots of %lld walkers x %d coordinates exceeds the %lld bytes one call may keep "
                       "on the device; the largest nkeep for this ensemble is %lld (raise thin)", name, (long long)nkeep, (long long)n, ctx->ndim,
                       (long long)kEnsMaxChainBytes, (long long)(kEnsMaxChainBytes / per));
    return MCALF_OK;
}

// What a failed launch of a kernel of ens_kernels.hip is reported as.
constexpr char kEnsLaunch[] = "hipLaunchKernel(ens_kernel_ptr(k), dim3(grid), dim3(kEnsWave), args, 0, stream)";

// The call over `n` device rows on `stream`: issued in one go, nothing is read back.
int run_ens(mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_ens_opts& o, hipStream_t stream) {
    if (n <= 0) return MCALF_OK;
    const size_t nb = (size_t)n, m = nb / 2, ndim = (size_t)ctx->ndim;
    int rc;
    if ((rc = grow(ctx, ctx->enb[mcalf_ctx::kEnY], m * ndim)) || (rc = grow(ctx, ctx->enb[mcalf_ctx::kEnLY], m)) ||
        (rc = grow(ctx, ctx->enb[mcalf_ctx::kEnAux], m * kEnsAux)) || (rc = grow(ctx, ctx->ens_inside, m)))
        return rc;
    EnsArgs a = {};
    a.U0 = r.U0; a.U = r.U; a.L = r.logL; a.status = r.status; a.naccept = r.naccept;
    a.Y = ctx->enb[mcalf_ctx::kEnY]; a.LY = ctx->enb[mcalf_ctx::kEnLY]; a.aux = ctx->enb[mcalf_ctx::kEnAux]; a.inside = ctx->ens_inside;
    a.seed = o.seed; a.scale = o.scale; a.n = (int)n; a.m = (int)m; a.ndim = ctx->ndim; a.move = o.move;
    const dim3 all((unsigned)n), half((unsigned)m), wave(kEnsWave);
    if ((rc = launch_block(ctx, ens_kernel_ptr(kEnsStart), a, all, wave, stream, kEnsLaunch)) || (rc = cube_logl(ctx, a.U, a.L, n, stream))) return rc;
    const size_t slotU = nb * ndim;
    for (int i = 0; i < o.nsteps; ++i) {
        const bool keep = (i + 1) % o.thin == 0;
        const size_t slot = keep ? (size_t)((i + 1) / o.thin - 1) : 0;
        for (int h = 0; h < 2; ++h) {
            a.half = h; a.step = 2 * (o.first_iter + (uint64_t)i) + (uint64_t)h;
            a.keep = keep && h == 1 && (r.CU || r.CL) ? 1 : 0;
            a.CU = a.keep && r.CU ? r.CU + slot * slotU : nullptr;
            a.CL = a.keep && r.CL ? r.CL + slot * nb : nullptr;
            if ((rc = launch_block(ctx, ens_kernel_ptr(kEnsPropose), a, half, wave, stream, kEnsLaunch)) || (rc = cube_logl(ctx, a.Y, a.LY, (int64_t)m, stream)) ||
                (rc = launch_block(ctx, ens_kernel_ptr(kEnsDecide), a, half, wave, stream, kEnsLaunch)))
                return rc;
        }
    }
    if (r.theta) return cube_to_theta(ctx, r.U, r.theta, n, stream);      // the transformed rows of the walkers
    return MCALF_OK;
}

// The host entry's call: the options, the chain arrays the caller wants, and the chain itself (the CU slots, then the CL slots),
// which lives as long as the call.
struct EnsCall { const mcalf_ens_opts* o; size_t nCU, nCL; DevBuf<double> chain; };
enum EnsCol { kColU0, kColU, kColTheta, kColL, kColStatus, kColNaccept, kColCU, kColCL, kEnsCols };

// The host entry's device driver (host_staged.cpp: run_staged); columns in the order of EnsCol, the chain's two its own.
int ens_body(mcalf_ctx* ctx, void** dev, int64_t n, hipStream_t stream, void* arg) {
    EnsCall* c = static_cast<EnsCall*>(arg);
    if (c->nCU + c->nCL > 0 && hipMalloc((void**)&c->chain.p, (c->nCU + c->nCL) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        c->chain.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "mcalf_ensemble_batch: no device memory for the chain of %zu slots (%.1f MB); raise thin",
                       (size_t)(c->o->nsteps / c->o->thin), (double)(c->nCU + c->nCL) * 8e-6);
    }
    dev[kColCU] = c->nCU ? c->chain.p : nullptr;
    dev[kColCL] = c->nCL ? c->chain.p + c->nCU : nullptr;
    const EnsRows d = {(const double*)dev[kColU0], (double*)dev[kColU], (double*)dev[kColTheta], (double*)dev[kColL], (int32_t*)dev[kColStatus],
                       (int32_t*)dev[kColNaccept], (double*)dev[kColCU], (double*)dev[kColCL]};
    const int rc = run_ens(ctx, d, n, *c->o, stream);
    if (rc) (void)hipStreamSynchronize(stream);           // (the chain is freed behind the stream)
    return rc;
}

// The walkers have to meet on one device: a multi-device context's first.
int ens_host(mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_ens_opts& o) {
    const size_t d = sizeof(double), i = sizeof(int32_t), ndim = (size_t)ctx->ndim, nkeep = (size_t)(o.nsteps / o.thin);
    EnsCall call = {&o, r.CU ? nkeep * (size_t)n * ndim : 0, r.CL ? nkeep * (size_t)n : 0, {}};      // (the chain is released when the call returns)
    StagePlan plan = {{stage_in(r.U0, d, ndim), stage_out(r.U, d, ndim), stage_out(r.theta, d, ndim), stage_out(r.logL, d, 1), stage_out(r.status, i, 1),
                       stage_out(r.naccept, i, 1), stage_out(r.CU, d, call.nCU, false, true), stage_out(r.CL, d, call.nCL, false, true)},
                      kEnsCols, n, kStageFirstDevice, kColU0, kColU, ens_body, &call};
    plan.cols[kColCU].present = call.nCU > 0;             // (a call that keeps no slot has no chain)
    plan.cols[kColCL].present = call.nCL > 0;
    return run_staged(ctx, plan);
}

}  // namespace

extern "C" int mcalf_ensemble_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const mcalf_ens_opts* opts, double* U, double* theta,
                                    double* logL, int32_t* status, int32_t* naccept, double* CU, double* CL) {
    const EnsRows r = {U0, U, theta, logL, status, naccept, CU, CL};
    const int rc = ens_check(ctx, "mcalf_ensemble_batch", r, nwalkers, opts);
    if (rc) return rc;
    if (nwalkers == 0) return MCALF_OK;
    return ens_host(ctx, r, nwalkers, *opts);
}

extern "C" int mcalf_ensemble_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const mcalf_ens_opts* opts, double* dU,
                                           double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept, double* dCU, double* dCL,
                                           void* stream) {
    const EnsRows r = {dU0, dU, dtheta, dlogL, dstatus, dnaccept, dCU, dCL};
    const int rc = ens_check(ctx, "mcalf_ensemble_batch_device", r, nwalkers, opts);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_ensemble_batch_device");
    if (nwalkers == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_ens(ctx, r, nwalkers, *opts, (hipStream_t)stream);
}
