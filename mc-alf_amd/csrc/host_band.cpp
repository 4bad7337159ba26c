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
    const dim3 moment_grid((unsigned)((size_t)nblocks * a.nstrips)), pixel_grid((unsigned)((npix + 255) / 256));
    if (batch > 0 && (rc = LAUNCH_BLOCK(ctx, band_kernel_ptr(kBandSum), a, moment_grid, dim3(kBandMomentThreads), stream))) return rc;
    if ((rc = LAUNCH_BLOCK(ctx, band_kernel_ptr(kBandMean), a, pixel_grid, dim3(256), stream))) return rc;
    if (a.var) {
        if (batch > 0 && (rc = LAUNCH_BLOCK(ctx, band_kernel_ptr(kBandSquares), a, moment_grid, dim3(kBandMomentThreads), stream))) return rc;
        if ((rc = LAUNCH_BLOCK(ctx, band_kernel_ptr(kBandVar), a, pixel_grid, dim3(256), stream))) return rc;
    }
    if (nq > 0) {
        if (batch > 0 && (rc = LAUNCH_BLOCK(ctx, band_kernel_ptr(kBandSelect), a, dim3((unsigned)(a.nstrips * nq)), dim3(kBandSelectThreads), stream))) return rc;
        if ((rc = LAUNCH_BLOCK(ctx, band_kernel_ptr(kBandInterp), a, dim3((unsigned)(((size_t)nq * npix + 255) / 256)), dim3(256), stream))) return rc;
    }
    return MCALF_OK;
}

// The host entry's call: what its device driver needs beyond the columns, and the model matrix, which lives as long as the call.
struct BandCall { int32_t targonly; const double* q; int32_t nq; DevBuf<double> M; };
enum { kColP, kColMean, kColVar, kColNvalid, kColQ };

int host_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    BandCall* c = static_cast<BandCall*>(arg);
    const size_t npix = (size_t)ctx->npix;
    if (hipMalloc((void**)&c->M.p, (size_t)rows * npix * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        c->M.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "mcalf_model_band_batch: no device memory for the %lld x %ld model matrix (%.1f MB); thin the chain",
                       (long long)rows, ctx->npix, (double)rows * (double)npix * 8e-6);
    }
    const BandOuts d = {(double*)dev[kColMean], (double*)dev[kColVar], (double*)dev[kColQ], (int64_t*)dev[kColNvalid]};
    return run_band(ctx, (const double*)dev[kColP], rows, c->targonly, c->q, c->nq, c->M, d, stream);
}

// All rows have to meet on one device: a multi-device context's first.  The results: mean, var, nvalid, Q[nq].
int run_host(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t targonly, const double* q, int32_t nq, const BandOuts& o) {
    BandCall call = {targonly, q, nq, {}};                // (M is released when the call returns, on every path)
    const size_t d = sizeof(double), npix = (size_t)ctx->npix;
    StagePlan plan = {{stage_in(P, d, (size_t)ctx->ndim), stage_out(o.mean, d, npix, false), stage_out(o.var, d, npix, false),
                       stage_out(o.nvalid, sizeof(int64_t), npix, false), stage_out(o.Q, d, (size_t)nq * npix, false)},
                      5, batch, kStageFirstDevice, kColP, -1, host_body, &call};
    return run_staged(ctx, plan);
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
