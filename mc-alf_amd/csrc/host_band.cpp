// Host side of the posterior-band kernels (band_kernels.hip): mcalf_model_band_batch and mcalf_model_band_batch_device.  One
// driver (run_band) has the likelihood's own launch write the model rows into the [batch][npix] matrix and issues the moment
// passes, the exact selection and the interpolation behind it.  The host entry owns the matrix for the length of the call
// only: an analysis call must not leave a context holding gigabytes.  What a context keeps are the per-pixel buffers and the
// per-block partials ([ceil(batch / kBandRowBlock)][npix]: 1 / 128 of the matrix).
#include <cmath>
#include <limits>

#include "band_args.h"
#include "host_ctx.h"

namespace {

struct BandOuts { double *mean, *var, *Q; int64_t* nvalid; };

int grow_buf(mcalf_ctx* ctx, int b, size_t elems) { return grow(ctx, ctx->bb[b], elems); }
int64_t band_nblocks(int64_t batch) { return (batch + kBandRowBlock - 1) / kBandRowBlock; }
int64_t band_max_batch(const mcalf_ctx* ctx) { return kBandMaxBytes / ((int64_t)ctx->npix * (int64_t)sizeof(double)); }

// Everything that is wrong with a call before any device work, and before a row of P is read; `name` is the entry that
// reports it.  `dM`: the device entry's workspace (need_M), else ignored.
int band_check(mcalf_ctx* ctx, const char* name, const double* P, int64_t batch, int32_t targonly, const double* q, int32_t nq,
               const BandOuts& o, bool need_M, const double* dM) {
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !P) return set_err(ctx, MCALF_ERR_INVALID, "%s: P is NULL", name);
    if (!o.mean && !o.var && !o.Q && !o.nvalid) return set_err(ctx, MCALF_ERR_INVALID, "%s: mean, var, Q and nvalid are all NULL", name);
    if (nq < 0 || nq > kBandMaxQ) return set_err(ctx, MCALF_ERR_INVALID, "%s: nq must be in [0, %d], got %d", name, kBandMaxQ, nq);
    if (nq > 0 && !q) return set_err(ctx, MCALF_ERR_INVALID, "%s: q is NULL with nq = %d", name, nq);
    if (nq > 0 && !o.Q) return set_err(ctx, MCALF_ERR_INVALID, "%s: Q is NULL with nq = %d", name, nq);
    if (nq == 0 && o.Q) return set_err(ctx, MCALF_ERR_INVALID, "%s: Q is given with nq = 0", name);
    for (int j = 0; j < nq; ++j)
        if (!std::isfinite(q[j]) || q[j] < 0.0 || q[j] > 1.0)
            return set_err(ctx, MCALF_ERR_INVALID, "%s: q[%d] = %g is not a quantile in [0, 1]", name, j, q[j]);
    if (targonly != 0 && targonly != 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: targonly must be 0 or 1, got %d", name, targonly);
    if (need_M && batch > 0 && !dM) return set_err(ctx, MCALF_ERR_INVALID, "%s: dM is NULL (the [batch][npix] workspace is the caller's)", name);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (batch > band_max_batch(ctx))
        return set_err(ctx, MCALF_ERR_RANGE, "%s: batch %lld x npix %ld doubles exceed the %lld-byte model matrix of one call; the largest "
                       "batch for this spectrum is %lld (thin the chain)", name, (long long)batch, ctx->npix, (long long)kBandMaxBytes,
                       (long long)band_max_batch(ctx));
    return MCALF_OK;
}

// The batch on `stream`, device pointers: the partials and per-pixel buffers (grown once: a later call of as many rows and
// quantiles or fewer allocates nothing), the model rows into dM by the likelihood's launch, then the band kernels; every
// kernel takes the argument block by value.  Count and mean always run (the later passes read them); the variance and the
// selection only when asked for -- no sum's order depends on that.  batch == 0: the combine and interpolation kernels
// alone, which then write NaN and 0.
int run_band(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t targonly, const double* q, int32_t nq, double* dM,
             const BandOuts& o, hipStream_t stream) {
    const size_t npix = (size_t)ctx->npix;
    const int64_t nblocks = band_nblocks(batch);
    int rc;
    if ((rc = grow_buf(ctx, mcalf_ctx::kBbPart, 2 * (size_t)nblocks * npix)) || (rc = grow_buf(ctx, mcalf_ctx::kBbMean, npix)) ||
        (rc = grow_buf(ctx, mcalf_ctx::kBbCount, npix)) || (rc = grow_buf(ctx, mcalf_ctx::kBbSel, 2 * (size_t)nq * npix)))
        return rc;
    if (batch > 0) {
        LaunchReq m(kModeModel, dP, batch, stream);
        m.targonly = targonly; m.d_model = dM;
        if ((rc = launch(ctx, m))) return rc;
    }
    BandArgs a = {};
    a.M = dM;
    a.part = ctx->bb[mcalf_ctx::kBbPart];
    a.pcnt = reinterpret_cast<long long*>(a.part + (size_t)nblocks * npix);
    a.mean = o.mean ? o.mean : ctx->bb[mcalf_ctx::kBbMean].p;
    a.var = o.var;
    a.nvalid = o.nvalid ? reinterpret_cast<long long*>(o.nvalid) : reinterpret_cast<long long*>(ctx->bb[mcalf_ctx::kBbCount].p);
    a.sel = ctx->bb[mcalf_ctx::kBbSel];
    a.Q = o.Q;
    a.batch = batch;
    a.npix = (int)npix; a.nstrips = (int)((npix + kBandStrip - 1) / kBandStrip); a.nblocks = (int)nblocks; a.nq = nq;
    for (int j = 0; j < nq; ++j) a.q[j] = q[j];
    void* args[] = {(void*)&a};
    const dim3 moment_grid((unsigned)((size_t)nblocks * a.nstrips)), pixel_grid((unsigned)((npix + 255) / 256));
    if (batch > 0) HIP_TRY(ctx, hipLaunchKernel(band_kernel_ptr(kBandSum), moment_grid, dim3(kBandMomentThreads), args, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel(band_kernel_ptr(kBandMean), pixel_grid, dim3(256), args, 0, stream));
    if (a.var) {
        if (batch > 0) HIP_TRY(ctx, hipLaunchKernel(band_kernel_ptr(kBandSquares), moment_grid, dim3(kBandMomentThreads), args, 0, stream));
        HIP_TRY(ctx, hipLaunchKernel(band_kernel_ptr(kBandVar), pixel_grid, dim3(256), args, 0, stream));
    }
    if (nq > 0) {
        if (batch > 0) HIP_TRY(ctx, hipLaunchKernel(band_kernel_ptr(kBandSelect), dim3((unsigned)(a.nstrips * nq)), dim3(kBandSelectThreads), args, 0, stream));
        HIP_TRY(ctx, hipLaunchKernel(band_kernel_ptr(kBandInterp), dim3((unsigned)(((size_t)nq * npix + 255) / 256)), dim3(256), args, 0, stream));
    }
    return MCALF_OK;
}

int run_host(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t targonly, const double* q, int32_t nq, const BandOuts& o) {
    if (is_multi(ctx)) {              // all rows have to meet on one device: the first entry's, bit for bit a single-device call
        mcalf_ctx* sub = ctx->subs[0];
        ctx->multi_last_active = 1;
        const int rc = run_host(sub, P, batch, targonly, q, nq, o);
        return rc ? set_err(ctx, rc, "device entry 0 (HIP device %d): %s", sub->device, sub->err.c_str()) : MCALF_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_HOST_STAGED, is_pinned_host(P), false);
    const size_t npix = (size_t)ctx->npix, nP = (size_t)batch * ctx->ndim;
    DevBuf<double> M;                                     // released when the call returns, on every path
    if (hipMalloc((void**)&M.p, (size_t)batch * npix * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        M.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "mcalf_model_band_batch: no device memory for the %lld x %ld model matrix (%.1f MB); thin the chain",
                       (long long)batch, ctx->npix, (double)batch * (double)npix * 8e-6);
    }
    int rc;
    // staging of the results: mean, var, nvalid, Q[nq]
    if ((rc = grow_buf(ctx, mcalf_ctx::kBbP, nP)) || (rc = grow_buf(ctx, mcalf_ctx::kBbOut, (3 + (size_t)nq) * npix))) return rc;
    double* out = ctx->bb[mcalf_ctx::kBbOut];
    BandOuts d = {o.mean ? out : nullptr, o.var ? out + npix : nullptr, o.Q ? out + 3 * npix : nullptr,
                  o.nvalid ? reinterpret_cast<int64_t*>(out + 2 * npix) : nullptr};
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bb[mcalf_ctx::kBbP], P, nP * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_band(ctx, ctx->bb[mcalf_ctx::kBbP], batch, targonly, q, nq, M, d, ctx->stream))) return rc;
    if (o.mean) HIP_TRY(ctx, hipMemcpyAsync(o.mean, d.mean, npix * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (o.var) HIP_TRY(ctx, hipMemcpyAsync(o.var, d.var, npix * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (o.nvalid) HIP_TRY(ctx, hipMemcpyAsync(o.nvalid, d.nvalid, npix * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (o.Q) HIP_TRY(ctx, hipMemcpyAsync(o.Q, d.Q, (size_t)nq * npix * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCALF_OK;
}

}  // namespace

extern "C" int mcalf_model_band_batch(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t targonly, const double* q, int32_t nq,
                                      double* mean, double* var, double* Q, int64_t* nvalid) {
    const BandOuts o = {mean, var, Q, nvalid};
    const int rc = band_check(ctx, "mcalf_model_band_batch", P, batch, targonly, q, nq, o, false, nullptr);
    if (rc) return rc;
    if (batch == 0) {                                     // no row: NaN everywhere, no valid entry (the caller's arrays, no device work)
        const size_t npix = (size_t)ctx->npix;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (mean) std::fill(mean, mean + npix, nan);
        if (var) std::fill(var, var + npix, nan);
        if (Q) std::fill(Q, Q + (size_t)nq * npix, nan);
        if (nvalid) std::fill(nvalid, nvalid + npix, (int64_t)0);
        return MCALF_OK;
    }
    return run_host(ctx, P, batch, targonly, q, nq, o);
}

extern "C" int mcalf_model_band_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t targonly, const double* q, int32_t nq,
                                             double* dM, double* dmean, double* dvar, double* dQ, int64_t* dnvalid, void* stream) {
    const BandOuts o = {dmean, dvar, dQ, dnvalid};
    const int rc = band_check(ctx, "mcalf_model_band_batch_device", dP, batch, targonly, q, nq, o, true, dM);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_model_band_batch_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_band(ctx, dP, batch, targonly, q, nq, dM, o, (hipStream_t)stream);
}
