// Host side of the fit kernels (fit_kernels.hip): the Fisher product J^T W J v on the device (mcalf_fisher_matvec_batch) and
// the batched Levenberg-Marquardt maximisation of logL built on it (mcalf_maximize_batch).  Both are drivers over
// host_grad.cpp's products (run_product: gradient, JVP, VJP) -- no Voigt code of their own -- and both run row block by row
// block inside ONE context-owned [rows][npix] workspace sized by the gradient driver's rule: rows * npix * 8 bytes within
// kGradChunkBytes, at most 65535 rows.  Nothing dense is formed: the fit solves its damped normal equations by conjugate
// gradients, one Fisher product per CG iteration.
#include <cmath>

#include "fit_args.h"
#include "host_ctx.h"

namespace {

int grow_buf(mcalf_ctx* ctx, int b, size_t elems) { return grow(ctx, ctx->fb[b], elems); }

int64_t fit_max_rows(const mcalf_ctx* ctx) {
    return std::min<int64_t>(65535, std::max<int64_t>(1, (int64_t)kGradChunkBytes / ((int64_t)ctx->npix * (int64_t)sizeof(double))));
}

// W [npix] of the Fisher product, built once per context: 1 / err^2 on the pixels whose logL term nansum keeps (the term
// err^-2 flux^2 - log err^-2 is not NaN), 0 elsewhere -- in host arithmetic, so that W has the bits numpy gives it.
int ensure_w(mcalf_ctx* ctx) {
    if (ctx->d_fitw.p) return MCALF_OK;
    const size_t npix = (size_t)ctx->npix;
    std::vector<double> flux(npix), err(npix), w(npix);
    HIP_TRY(ctx, hipMemcpy(flux.data(), ctx->d_obj, npix * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(err.data(), ctx->d_err, npix * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i) {
        const double wi = 1.0 / (err[i] * err[i]);
        const double term = wi * (flux[i] * flux[i]) - std::log(wi);
        w[i] = std::isnan(term) ? 0.0 : wi;
    }
    DevBuf<double> buf;
    int rc = grow(ctx, buf, npix);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(buf.p, w.data(), npix * sizeof(double), hipMemcpyHostToDevice));
    std::swap(ctx->d_fitw.p, buf.p);
    std::swap(ctx->d_fitw.cap, buf.cap);
    return MCALF_OK;
}

int launch_fit(mcalf_ctx* ctx, FitKernel k, const FitArgs& a, hipStream_t stream) {
    if (k == kFitWeight)
        return LAUNCH_BLOCK(ctx, fit_kernel_ptr(k), a, dim3((unsigned)((a.npix + kFitPixBlock - 1) / kFitPixBlock), (unsigned)a.nrows),
                            dim3(kFitPixBlock), stream);
    return LAUNCH_BLOCK(ctx, fit_kernel_ptr(k), a, dim3((unsigned)a.nrows), dim3(kFitWave), stream);
}

// FV = J^T W J V over `n` <= fit_max_rows device rows: the JVP into the workspace, the weight, the VJP of the workspace.
int fisher_block(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t n, double* dFV, hipStream_t stream) {
    double* dM = ctx->fb[mcalf_ctx::kFbDM];
    int rc;
    if ((rc = run_product(ctx, kProdJvp, {dP, dV, dM, nullptr}, n, stream))) return rc;
    FitArgs w = {};
    w.dM = dM; w.W = ctx->d_fitw; w.nrows = (int)n; w.npix = (int)ctx->npix;
    if ((rc = launch_fit(ctx, kFitWeight, w, stream))) return rc;
    return run_product(ctx, kProdVjp, {dP, dM, dFV, nullptr}, n, stream);
}

// What a Fisher product or a fit of row blocks of `rows` rows needs beyond the products' own workspaces (grown once).
int fisher_prepare(mcalf_ctx* ctx, int64_t rows) {
    int rc = grow_buf(ctx, mcalf_ctx::kFbDM, (size_t)rows * (size_t)ctx->npix);
    return rc ? rc : ensure_w(ctx);
}

int run_fisher(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dFV, hipStream_t stream) {
    const int64_t chunk = fit_max_rows(ctx);
    int rc = fisher_prepare(ctx, std::min(batch, chunk));
    if (rc) return rc;
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        const size_t o = (size_t)row0 * ctx->ndim;
        if ((rc = fisher_block(ctx, dP + o, dV + o, std::min(chunk, batch - row0), dFV + o, stream))) return rc;
    }
    return MCALF_OK;
}

int fisher_check(mcalf_ctx* ctx, const char* name, const double* P, const double* V, int64_t batch, const double* FV) {
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !P) return set_err(ctx, MCALF_ERR_INVALID, "%s: P is NULL", name);
    if (batch > 0 && !V) return set_err(ctx, MCALF_ERR_INVALID, "%s: V is NULL", name);
    if (batch > 0 && !FV) return set_err(ctx, MCALF_ERR_INVALID, "%s: FV is NULL", name);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    return MCALF_OK;
}

// The host entry's device driver (host_staged.cpp: run_staged); columns P, V, FV.
int fisher_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void*) {
    return run_fisher(ctx, (const double*)dev[0], (const double*)dev[1], rows, (double*)dev[2], stream);
}

int fisher_host(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* FV) {
    const size_t d = sizeof(double), ndim = (size_t)ctx->ndim;
    StagePlan plan = {{stage_in(P, d, ndim), stage_in(V, d, ndim), stage_out(FV, d, ndim)}, 3, batch, kStageCutRows, 0, 2, fisher_body, nullptr};
    return run_staged(ctx, plan);
}

// ---- the fit ---------------------------------------------------------------------------------------------------------------

struct FitRows { const double* P0; double *P, *logL; int32_t *status, *niter; };

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.
int fit_check(mcalf_ctx* ctx, const char* name, const FitRows& r, int64_t batch, const mcalf_fit_opts* o) {
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !r.P0) return set_err(ctx, MCALF_ERR_INVALID, "%s: P0 is NULL", name);
    if (batch > 0 && !r.P) return set_err(ctx, MCALF_ERR_INVALID, "%s: P is NULL", name);
    if (batch > 0 && !r.logL) return set_err(ctx, MCALF_ERR_INVALID, "%s: logL is NULL", name);
    if (batch > 0 && !r.status) return set_err(ctx, MCALF_ERR_INVALID, "%s: status is NULL", name);
    if (batch > 0 && !r.niter) return set_err(ctx, MCALF_ERR_INVALID, "%s: niter is NULL", name);
    if (o->max_iter < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: max_iter must be >= 0, got %d", name, o->max_iter);
    if (o->cg_iters < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: cg_iters must be >= 0, got %d", name, o->cg_iters);
    if (o->rows_per_block < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: rows_per_block must be >= 0, got %d", name, o->rows_per_block);
    if (!std::isfinite(o->lambda0) || !(o->lambda0 > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: lambda0 must be finite and > 0, got %g", name, o->lambda0);
    if (!std::isfinite(o->ftol) || !(o->ftol >= 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: ftol must be finite and >= 0, got %g", name, o->ftol);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the fit works inside its box)", name);
    const std::vector<double>& box = is_multi(ctx) ? ctx->subs[0]->h_prior : ctx->h_prior;
    for (int k = 0; k < ctx->ndim; ++k) {
        const double lo = box[k], hi = box[ctx->ndim + k];
        if (!std::isfinite(lo) || !std::isfinite(hi)) return set_err(ctx, MCALF_ERR_INVALID, "%s: prior bound %d is not finite (lo %g, hi %g)", name, k, lo, hi);
        if (lo > hi) return set_err(ctx, MCALF_ERR_INVALID, "%s: prior box has lo > hi at parameter %d (%g > %g)", name, k, lo, hi);
    }
    return MCALF_OK;
}

// The fit of `batch` device rows on `stream`, row block by row block; each block runs its whole fit.  poll: after every outer
// iteration the host reads the counter of live rows (4 bytes) and leaves the block's loop at 0 -- finished rows are carried,
// so the rows' bits are those of the unconditional max_iter iterations the device entry runs.
int run_fit(mcalf_ctx* ctx, const FitRows& r, int64_t batch, const mcalf_fit_opts& o, hipStream_t stream, bool poll) {
    if (batch <= 0) return MCALF_OK;
    int64_t block = fit_max_rows(ctx);
    if (o.rows_per_block > 0) block = std::min<int64_t>(block, o.rows_per_block);
    const size_t rows = (size_t)std::min(batch, block), ndim = (size_t)ctx->ndim;
    int rc;
    if ((rc = fisher_prepare(ctx, (int64_t)rows))) return rc;
    for (int b = mcalf_ctx::kFbT; b <= mcalf_ctx::kFbFV; ++b)
        if ((rc = grow_buf(ctx, b, rows * ndim))) return rc;
    if ((rc = grow_buf(ctx, mcalf_ctx::kFbScal, rows * kFitScal)) || (rc = grow(ctx, ctx->fit_int, rows * (1 + ndim))) ||
        (rc = grow(ctx, ctx->d_fit_live, 1)))
        return rc;
    const DevBuf<double>* fb = ctx->fb;
    const int cg = o.cg_iters > 0 ? o.cg_iters : ctx->ndim;
    for (int64_t row0 = 0; row0 < batch; row0 += block) {
        const int64_t n = std::min(block, batch - row0);
        const size_t o0 = (size_t)row0 * ndim;
        FitArgs a = {};
        a.P0 = r.P0 + o0; a.th = r.P + o0; a.L = r.logL + row0; a.status = r.status + row0; a.niter = r.niter + row0;
        a.lo = ctx->d_prior; a.hi = ctx->d_prior + ndim;
        a.T = fb[mcalf_ctx::kFbT]; a.G = fb[mcalf_ctx::kFbG]; a.GT = fb[mcalf_ctx::kFbGT]; a.gu = fb[mcalf_ctx::kFbGu];
        a.x = fb[mcalf_ctx::kFbX]; a.r = fb[mcalf_ctx::kFbR]; a.p = fb[mcalf_ctx::kFbPv]; a.V = fb[mcalf_ctx::kFbV]; a.FV = fb[mcalf_ctx::kFbFV];
        a.scal = fb[mcalf_ctx::kFbScal]; a.frozen = ctx->fit_int; a.pin = ctx->fit_int + rows; a.live = ctx->d_fit_live;
        a.nrows = (int)n; a.npix = (int)ctx->npix; a.lay = row_layout(ctx);
        a.lambda0 = o.lambda0; a.ftol = o.ftol;
        double* LT = a.scal + 3 * (size_t)n;
        if ((rc = launch_fit(ctx, kFitStart, a, stream)) || (rc = run_product(ctx, kProdGrad, {a.th, nullptr, a.G, a.L}, n, stream)) ||
            (rc = launch_fit(ctx, kFitStarted, a, stream)))
            return rc;
        for (int it = 0; it < o.max_iter; ++it) {
            if (poll) HIP_TRY(ctx, hipMemsetAsync(a.live, 0, sizeof(unsigned int), stream));
            if ((rc = launch_fit(ctx, kFitBegin, a, stream))) return rc;
            for (int j = 0; j < cg; ++j)
                if ((rc = fisher_block(ctx, a.th, a.V, n, fb[mcalf_ctx::kFbFV], stream)) || (rc = launch_fit(ctx, kFitCg, a, stream))) return rc;
            if ((rc = launch_fit(ctx, kFitTrial, a, stream)) || (rc = run_product(ctx, kProdGrad, {a.T, nullptr, a.GT, LT}, n, stream)) ||
                (rc = launch_fit(ctx, kFitAccept, a, stream)))
                return rc;
            if (poll) {
                unsigned int live = 0;
                HIP_TRY(ctx, hipMemcpyAsync(&live, a.live, sizeof(live), hipMemcpyDeviceToHost, stream));
                HIP_TRY(ctx, hipStreamSynchronize(stream));
                if (live == 0) break;
            }
        }
    }
    return MCALF_OK;
}

// The host entry's device driver (host_staged.cpp: run_staged); columns P0, P, logL, status, niter.
int fit_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    const FitRows d = {(const double*)dev[0], (double*)dev[1], (double*)dev[2], (int32_t*)dev[3], (int32_t*)dev[4]};
    return run_fit(ctx, d, rows, *static_cast<const mcalf_fit_opts*>(arg), stream, true);
}

int fit_host(mcalf_ctx* ctx, const FitRows& r, int64_t batch, const mcalf_fit_opts& o) {
    const size_t d = sizeof(double), i = sizeof(int32_t), ndim = (size_t)ctx->ndim;
    StagePlan plan = {{stage_in(r.P0, d, ndim), stage_out(r.P, d, ndim), stage_out(r.logL, d, 1), stage_out(r.status, i, 1), stage_out(r.niter, i, 1)},
                      5, batch, kStageCutRows, 0, 1, fit_body, const_cast<mcalf_fit_opts*>(&o)};
    return run_staged(ctx, plan);
}

}  // namespace

extern "C" int mcalf_fisher_matvec_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* FV) {
    const int rc = fisher_check(ctx, "mcalf_fisher_matvec_batch", P, V, batch, FV);
    if (rc || batch == 0) return rc;
    return fisher_host(ctx, P, V, batch, FV);
}

extern "C" int mcalf_fisher_matvec_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dFV, void* stream) {
    const int rc = fisher_check(ctx, "mcalf_fisher_matvec_batch_device", dP, dV, batch, dFV);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_fisher_matvec_batch_device");
    if (batch == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_fisher(ctx, dP, dV, batch, dFV, (hipStream_t)stream);
}

extern "C" int mcalf_maximize_batch(mcalf_ctx* ctx, const double* P0, int64_t batch, const mcalf_fit_opts* opts, double* P, double* logL,
                                    int32_t* status, int32_t* niter) {
    const FitRows r = {P0, P, logL, status, niter};
    const int rc = fit_check(ctx, "mcalf_maximize_batch", r, batch, opts);
    if (rc || batch == 0) return rc;
    return fit_host(ctx, r, batch, *opts);
}

extern "C" int mcalf_maximize_batch_device(mcalf_ctx* ctx, const double* dP0, int64_t batch, const mcalf_fit_opts* opts, double* dP,
                                           double* dlogL, int32_t* dstatus, int32_t* dniter, void* stream) {
    const FitRows r = {dP0, dP, dlogL, dstatus, dniter};
    const int rc = fit_check(ctx, "mcalf_maximize_batch_device", r, batch, opts);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_maximize_batch_device");
    if (batch == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_fit(ctx, r, batch, *opts, (hipStream_t)stream, false);
}
