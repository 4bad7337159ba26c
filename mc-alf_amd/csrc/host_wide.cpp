// libmcalf_hip.so, host side: the launch of a WIDE-LSF context (ctx->wide: the LSF half-width does not fit a workgroup tile) --
// a convolution-free fused launch, then the wide kernels of kernels.hip convolve from HBM.
#include "host_ctx.h"

// Live points per pass of a wide-LSF launch (launch_wide): each of its scratch buffers -- unconvolved spectra, taps -- stays
// below 512 MB; 0 when a single live point does not fit.
int64_t wide_rows_per_pass(const mcalf_ctx* ctx, int64_t batch) {
    constexpr size_t kScratchBytes = (size_t)512 << 20;
    const size_t per_row = sizeof(double) * (size_t)std::max<int64_t>(ctx->npix, 2 * (int64_t)ctx->wide_n_cap + 1);
    if (per_row > kScratchBytes) return 0;
    return std::min<int64_t>(batch, std::min<int64_t>(65535, std::max<int64_t>(1, (int64_t)(kScratchBytes / per_row))));
}

// The scratch of one pass of `rows` live points: unconvolved spectra, taps, headers; the block sums of the likelihood terms
// (partials) and the rows of mcalf_onecomp_batch (onecomp_rows) where the mode needs them -- mcalf_reserve provisions all.
int grow_wide_ws(mcalf_ctx* ctx, int64_t rows, bool partials, bool onecomp_rows) {
    const int nblocks = (int)((ctx->npix + kWideBlockPix - 1) / kWideBlockPix);
    int rc;
    if ((rc = grow(ctx, ctx->d_wide, (size_t)rows * ctx->npix))) return rc;
    if ((rc = grow(ctx, ctx->d_wtaps, (size_t)rows * (2 * (size_t)ctx->wide_n_cap + 1)))) return rc;
    if ((rc = grow(ctx, ctx->d_whdr, (size_t)rows))) return rc;
    if (partials && (rc = grow(ctx, ctx->d_wpartial, (size_t)rows * nblocks * 4))) return rc;
    if (onecomp_rows && (rc = grow(ctx, ctx->d_wrows, (size_t)rows * 5))) return rc;
    return MCALF_OK;
}

// A batch of a WIDE-LSF context (ctx->wide: the LSF half-width does not fit a workgroup tile; numpy boundary): per pass of
// at most `rows` live points -- bounded scratch -- (1) the fused kernel WITHOUT convolution and continuum (make_kargs:
// wide_stage1) writes the unconvolved spectra into d_wide, (2) mcalf_wide_taps_kernel forms every live point's taps,
// (3) mcalf_wide_conv_kernel convolves periodically from HBM, applies the continuum and writes the model rows and / or the
// block sums of the likelihood terms, (4) mcalf_finalize_kernel adds those up.  Same entry points, same error values
// (a resolution beyond specres_max: NaN model, logL = -inf, chi2 = +inf); hires_fitter.py:445-464.
int launch_wide(mcalf_ctx* ctx, const LaunchReq& q) {
    const int mode = q.mode, rowlen = q.rowlen(ctx);
    const hipStream_t stream = q.stream;
    const int64_t batch = q.batch, npix = ctx->npix, tapw = 2 * (int64_t)ctx->wide_n_cap + 1;
    const bool jax = ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX, reduces = q.reduces();
    const int64_t rows = wide_rows_per_pass(ctx, batch);
    if (rows < 1) return set_err(ctx, MCALF_ERR_RANGE, "wide LSF: one live point exceeds the scratch of a pass");
    const int nblocks = (int)((npix + kWideBlockPix - 1) / kWideBlockPix);
    int rc;
    if ((rc = launch_preflight(ctx, kModeModel, rows))) return rc;
    if ((rc = grow_wide_ws(ctx, rows, reduces, mode == kModeOneComp))) return rc;
    ctx->last.row_blocks = (int32_t)((batch + rows - 1) / rows);
    // per pass: the fused launch writes d_wide (this mode's rows or the model's; no scalar), the wide kernels the caller's arrays
    LaunchReq fused = q, conv = q;
    if (mode != kModeOneComp) fused.mode = kModeModel;
    fused.d_out = nullptr; fused.d_model = ctx->d_wide; conv.d_theta = nullptr;
    for (int64_t r0 = 0; r0 < batch; r0 += rows) {
        const int64_t n = std::min(rows, batch - r0);
        const double* P0 = q.dP + (size_t)r0 * rowlen;
        const double* P1 = P0;
        if (mode == kModeOneComp) {                           // (the fused kernel reads this mode's continuum from the row: rows with 1)
            double* wr = ctx->d_wrows;
            long cnt = (long)n;
            void* kargs[] = {(void*)&P0, (void*)&wr, (void*)&cnt};
            HIP_TRY(ctx, hipLaunchKernel(wide_rows_kernel_ptr(), dim3((unsigned)((n * 5 + 255) / 256)), dim3(256), kargs, 0, stream));
            P1 = wr;
        }
        fused.dP = P1;
        fused.d_theta = q.d_theta ? q.d_theta + (size_t)r0 * ctx->ndim : nullptr;
        if ((rc = launch_range(ctx, fused, 0, n, 0, stream, r0 == 0, kWideFused))) return rc;
        conv.dP = P0;
        conv.d_out = q.d_out ? q.d_out + r0 : nullptr;
        conv.d_model = q.d_model ? q.d_model + (size_t)r0 * npix : nullptr;
        KArgs a = make_kargs(ctx, conv, 0, n, 0, kWideKernels);
        a.partial = ctx->d_wpartial;
        double* taps = ctx->d_wtaps;
        const double* taps_c = taps;
        const double* flux = ctx->d_wide;
        SampleHdr* hdr = ctx->d_whdr;
        const SampleHdr* hdr_c = hdr;
        long stride = (long)tapw;
        int nb = nblocks;
        {
            void* kargs[] = {(void*)&a, (void*)&taps, (void*)&stride, (void*)&hdr};
            HIP_TRY(ctx, hipLaunchKernel(wide_taps_kernel_ptr(jax), dim3((unsigned)n), dim3(kWideBlockThreads), kargs, 0, stream));
        }
        {
            void* kargs[] = {(void*)&a, (void*)&flux, (void*)&taps_c, (void*)&stride, (void*)&hdr_c, (void*)&nb};
            HIP_TRY(ctx, hipLaunchKernel(wide_conv_kernel_ptr(jax), dim3((unsigned)nblocks, (unsigned)n), dim3(kWideBlockThreads), kargs, 0, stream));
        }
        if (reduces && (rc = launch_finalize(ctx, a, n, mode, stream, nblocks))) return rc;   // (nblocks partials per live point)
    }
    return MCALF_OK;
}
