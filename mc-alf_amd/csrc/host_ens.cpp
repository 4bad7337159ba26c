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

int launch_ens(mcalf_ctx* ctx, EnsKernel k, const EnsArgs& a, hipStream_t stream, unsigned grid) {
    void* args[] = {(void*)&a};
    HIP_TRY(ctx, hipLaunchKernel(ens_kernel_ptr(k), dim3(grid), dim3(kEnsWave), args, 0, stream));
    return MCALF_OK;
}

// logL of the `n` rows at Y into LY, exactly what mcalf_loglike_cube_batch_device(Y) writes.
int trial_logl(mcalf_ctx* ctx, const double* Y, const double* LY, int64_t n, hipStream_t stream) {
    LaunchReq q(kModeLogL, Y, n, stream);
    q.d_out = const_cast<double*>(LY); q.from_cube = true;
    return launch(ctx, q);
}

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
    if ((rc = launch_ens(ctx, kEnsStart, a, stream, (unsigned)n)) || (rc = trial_logl(ctx, a.U, a.L, n, stream))) return rc;
    const size_t slotU = nb * ndim;
    for (int i = 0; i < o.nsteps; ++i) {
        const bool keep = (i + 1) % o.thin == 0;
        const size_t slot = keep ? (size_t)((i + 1) / o.thin - 1) : 0;
        for (int h = 0; h < 2; ++h) {
            a.half = h; a.step = 2 * (o.first_iter + (uint64_t)i) + (uint64_t)h;
            a.keep = keep && h == 1 && (r.CU || r.CL) ? 1 : 0;
            a.CU = a.keep && r.CU ? r.CU + slot * slotU : nullptr;
            a.CL = a.keep && r.CL ? r.CL + slot * nb : nullptr;
            if ((rc = launch_ens(ctx, kEnsPropose, a, stream, (unsigned)m)) || (rc = trial_logl(ctx, a.Y, a.LY, (int64_t)m, stream)) ||
                (rc = launch_ens(ctx, kEnsDecide, a, stream, (unsigned)m)))
                return rc;
        }
    }
    if (r.theta) {                                      // the transformed rows of the walkers, as the cube launch forms them
        const double *lo = ctx->d_prior, *hi = ctx->d_prior + ndim, *cube = r.U;
        long total = (long)(nb * ndim);
        int nd = ctx->ndim, slot = ctx->startind, as_int = ctx->prior_int;
        double* theta = r.theta;
        void* kargs[] = {(void*)&lo, (void*)&hi, (void*)&cube, (void*)&total, (void*)&nd, (void*)&slot, (void*)&as_int, (void*)&theta};
        HIP_TRY(ctx, hipLaunchKernel(scale_cube_kernel_ptr(), dim3((unsigned)((total + 255) / 256)), dim3(256), kargs, 0, stream));
    }
    return MCALF_OK;
}

int ens_host(mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_ens_opts& o) {
    if (is_multi(ctx)) {              // the walkers have to meet on one device: the first entry's, bit for bit a single-device call
        mcalf_ctx* sub = ctx->subs[0];
        ctx->multi_last_active = 1;
        const int rc = ens_host(sub, r, n, o);
        return rc ? set_err(ctx, rc, "device entry 0 (HIP device %d): %s", sub->device, sub->err.c_str()) : MCALF_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_HOST_STAGED, is_pinned_host(r.U0), is_pinned_host(r.U));
    const size_t nb = (size_t)n, nu = nb * ctx->ndim, nkeep = (size_t)(o.nsteps / o.thin);
    DevBuf<double>* b = ctx->enb;
    int rc;
    if ((rc = grow(ctx, b[mcalf_ctx::kEnU0], nu)) || (rc = grow(ctx, b[mcalf_ctx::kEnU], nu)) || (rc = grow(ctx, b[mcalf_ctx::kEnL], nb)) ||
        (r.theta && (rc = grow(ctx, b[mcalf_ctx::kEnTheta], nu))) || (rc = grow(ctx, ctx->ens_hst, 2 * nb)))
        return rc;
    DevBuf<double> chain;                                 // released when the call returns, on every path
    const size_t nCU = r.CU ? nkeep * nu : 0, nCL = r.CL ? nkeep * nb : 0;
    if (nCU + nCL > 0 && hipMalloc((void**)&chain.p, (nCU + nCL) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        chain.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "mcalf_ensemble_batch: no device memory for the chain of %zu slots (%.1f MB); raise thin",
                       nkeep, (double)(nCU + nCL) * 8e-6);
    }
    const EnsRows d = {b[mcalf_ctx::kEnU0], b[mcalf_ctx::kEnU], r.theta ? b[mcalf_ctx::kEnTheta].p : nullptr, b[mcalf_ctx::kEnL],
                       ctx->ens_hst, ctx->ens_hst + nb, nCU ? chain.p : nullptr, nCL ? chain.p + nCU : nullptr};
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(b[mcalf_ctx::kEnU0], r.U0, nu * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = run_ens(ctx, d, n, o, st))) { (void)hipStreamSynchronize(st); return rc; }      // (the chain is freed behind the stream)
    HIP_TRY(ctx, hipMemcpyAsync(r.U, d.U, nu * sizeof(double), hipMemcpyDeviceToHost, st));
    if (r.theta) HIP_TRY(ctx, hipMemcpyAsync(r.theta, d.theta, nu * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(r.logL, d.logL, nb * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(r.status, d.status, nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(r.naccept, d.naccept, nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nCU) HIP_TRY(ctx, hipMemcpyAsync(r.CU, d.CU, nCU * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nCL) HIP_TRY(ctx, hipMemcpyAsync(r.CL, d.CL, nCL * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MCALF_OK;
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
