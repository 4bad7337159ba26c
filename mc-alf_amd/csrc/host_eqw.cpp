// Host side of the equivalent-width kernels (eqw_kernels.hip): mcalf_eqw_batch and mcalf_eqw_batch_device.  One driver
// (run_eqw) issues set-up, pixel pass and finalize pass by pass over row blocks whose per-row workspaces stay within
// kGradChunkBytes and whose rows fit grid.y -- the derivative driver's rule (host_grad.cpp).  The wavelength steps dlam are a
// device array of the context, computed once in mcalf_create with numpy's two steps (hires_fitter.py:485-486).
#include "eqw_args.h"
#include "grad_args.h"
#include "host_ctx.h"

static_assert(kEqwIndexLayout == MCALF_EQW_LAYOUT && kEqwIndexAsWritten == MCALF_EQW_AS_WRITTEN, "the kernels' indexing codes are the ABI's");

namespace {

int eqw_ntiles(const mcalf_ctx* ctx) { return (int)((ctx->npix + kEqwTile - 1) / kEqwTile); }
int64_t eqw_nrec(const mcalf_ctx* ctx) { return (int64_t)ctx->ncompmax * ctx->nlines; }
int64_t eqw_ncells(const mcalf_ctx* ctx) { return (int64_t)(ctx->ncompmax + 1) * ctx->nlines; }
// doubles per row of the two per-row workspaces
int64_t recs_row(const mcalf_ctx* ctx) { return std::max<int64_t>(1, eqw_nrec(ctx)) * kEqwRec; }
int64_t part_row(const mcalf_ctx* ctx) { return (int64_t)eqw_ntiles(ctx) * eqw_ncells(ctx) * kEqwWaves; }

// Rows per pass: the workspaces of a pass within kGradChunkBytes, and the row on grid.y of the pixel kernel.
constexpr int64_t kEqwMaxRows = 65535;
int64_t eqw_chunk_rows(const mcalf_ctx* ctx) {
    const int64_t per_row = (recs_row(ctx) + part_row(ctx)) * (int64_t)sizeof(double);
    return std::min<int64_t>(kEqwMaxRows, std::max<int64_t>(1, (int64_t)kGradChunkBytes / per_row));
}

int grow_buf(mcalf_ctx* ctx, int b, size_t elems) { return grow(ctx, ctx->eb[b], elems); }

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.
int eqw_check(mcalf_ctx* ctx, const char* name, const double* P, int64_t batch, int32_t indexing, const double* Wcomp, const double* Wblend) {
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !P) return set_err(ctx, MCALF_ERR_INVALID, "%s: P is NULL", name);
    if (!Wcomp && !Wblend) return set_err(ctx, MCALF_ERR_INVALID, "%s: Wcomp and Wblend are both NULL", name);
    if (indexing != MCALF_EQW_LAYOUT && indexing != MCALF_EQW_AS_WRITTEN)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: indexing must be MCALF_EQW_LAYOUT (0) or MCALF_EQW_AS_WRITTEN (1), got %d", name, indexing);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (ctx->npix < 2)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: npix = %ld, an equivalent width needs a spectrum of at least 2 pixels "
                       "(dlambda[0] = wl[1] - wl[0], hires_fitter.py:485-486)", name, ctx->npix);
    return MCALF_OK;
}

// The batch on `stream`, device pointers: the workspaces of one pass (grown once: a later call of as many rows or fewer
// allocates nothing), then the three kernels pass by pass; every kernel takes the argument block by value.
int run_eqw(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t indexing, double* dWcomp, double* dWblend, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    const int64_t chunk = eqw_chunk_rows(ctx);
    const size_t rows = (size_t)std::min(batch, chunk);
    int rc;
    if ((rc = grow_buf(ctx, mcalf_ctx::kEbRecs, rows * (size_t)recs_row(ctx))) || (rc = grow_buf(ctx, mcalf_ctx::kEbPart, rows * (size_t)part_row(ctx))))
        return rc;
    EqwArgs a = {};
    a.nu = ctx->d_nu; a.dlam = ctx->d_dlam; a.lines = ctx->d_lines; a.tabs = ctx->d_tabs;
    a.recs = ctx->eb[mcalf_ctx::kEbRecs]; a.part = ctx->eb[mcalf_ctx::kEbPart];
    a.npix = (int)ctx->npix; a.ntiles = eqw_ntiles(ctx); a.indexing = indexing; a.lay = row_layout(ctx);
    const size_t nrec = (size_t)eqw_nrec(ctx), ncells = (size_t)eqw_ncells(ctx);
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        a.P = dP + (size_t)row0 * ctx->ndim;
        a.Wcomp = dWcomp ? dWcomp + (size_t)row0 * nrec : nullptr;
        a.Wblend = dWblend ? dWblend + (size_t)row0 * ctx->nlines : nullptr;
        a.nrows = (int)std::min(chunk, batch - row0);
        if ((rc = LAUNCH_BLOCK(ctx, eqw_kernel_ptr(kEqwSetup), a, dim3((unsigned)a.nrows), dim3(64), stream)) ||
            (rc = LAUNCH_BLOCK(ctx, eqw_kernel_ptr(kEqwPixel), a, dim3((unsigned)a.ntiles, (unsigned)a.nrows), dim3(kEqwBlock), stream)) ||
            (rc = LAUNCH_BLOCK(ctx, eqw_kernel_ptr(kEqwFinalize), a, dim3((unsigned)(((size_t)a.nrows * ncells + 255) / 256)), dim3(256), stream)))
            return rc;
    }
    return MCALF_OK;
}

// The host entry's device driver (host_staged.cpp: run_staged); columns P, Wcomp, Wblend.
int host_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    return run_eqw(ctx, (const double*)dev[0], rows, *static_cast<const int32_t*>(arg), (double*)dev[1], (double*)dev[2], stream);
}

int run_host(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t indexing, double* Wcomp, double* Wblend) {
    const size_t d = sizeof(double), nrec = (size_t)eqw_nrec(ctx);
    StagePlan plan = {{stage_in(P, d, (size_t)ctx->ndim), stage_out(Wcomp, d, nrec), stage_out(Wblend, d, (size_t)ctx->nlines)},
                      3, batch, kStageCutRows, 0, Wcomp ? 1 : 2, host_body, &indexing};
    plan.cols[1].present = Wcomp && nrec;                 // (a layout without components has no Wcomp rows)
    return run_staged(ctx, plan);
}

}  // namespace

// dlam[0] = wl[1] - wl[0], dlam[i] = wl[i] - wl[i-1]: np.diff, then np.insert(d, 0, d[0]) (hires_fitter.py:485-486).  A
// one-pixel spectrum has none (the entries refuse it).
int eqw_prepare(mcalf_ctx* ctx, const double* wl) {
    if (ctx->npix < 2) return MCALF_OK;
    std::vector<double> dlam((size_t)ctx->npix);
    for (long i = 1; i < ctx->npix; ++i) dlam[i] = wl[i] - wl[i - 1];
    dlam[0] = dlam[1];
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_dlam.p, dlam.size() * sizeof(double)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_dlam, dlam.data(), dlam.size() * sizeof(double), hipMemcpyHostToDevice));
    return MCALF_OK;
}

extern "C" int mcalf_eqw_batch(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t indexing, double* Wcomp, double* Wblend) {
    const int rc = eqw_check(ctx, "mcalf_eqw_batch", P, batch, indexing, Wcomp, Wblend);
    if (rc || batch == 0) return rc;
    return run_host(ctx, P, batch, indexing, Wcomp, Wblend);
}

extern "C" int mcalf_eqw_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t indexing, double* dWcomp, double* dWblend,
                                      void* stream) {
    const int rc = eqw_check(ctx, "mcalf_eqw_batch_device", dP, batch, indexing, dWcomp, dWblend);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_eqw_batch_device");
    if (batch == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_eqw(ctx, dP, batch, indexing, dWcomp, dWblend, (hipStream_t)stream);
}
