// Host side of the analytic gradient of logL (grad_kernels.hip): mcalf_loglike_grad_batch[_device] and
// mcalf_voigt_hjerting_grad.  logL itself comes from the likelihood's own launch (host_abi.cpp: launch), so the two
// entries agree on it bit for bit; the gradient kernels then run over row blocks whose per-row workspaces stay within
// kGradChunkBytes.  The model Jacobian's products with a vector, mcalf_model_jvp_batch[_device] and
// mcalf_model_vjp_batch[_device], run over the same row blocks and workspaces.  The Hessian-vector product of logL,
// mcalf_loglike_hvp_batch[_device], shares them too and adds three per-row workspaces, so its passes are cut smaller.
#include <cmath>

#include "grad_args.h"
#include "host_ctx.h"

namespace {

int grad_ntiles(const mcalf_ctx* ctx) { return (int)((ctx->npix + kGradBlock - 1) / kGradBlock); }
int grad_nslots(const mcalf_ctx* ctx) { return std::max(1, ctx->ncompmax * ctx->nlines + ctx->nfill); }
int grad_ncap(const mcalf_ctx* ctx) {
    return ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX ? ctx->jax_half : (ctx->wide ? ctx->wide_n_cap : ctx->n_cap);
}
int grad_tapcap(const mcalf_ctx* ctx) { return 2 * grad_ncap(ctx) + 1; }

// Rows per pass: EVERY per-row workspace of a pass (F, q, taps and their R derivative, records, partials) within
// kGradChunkBytes -- the taps of a wide-LSF context are thousands of doubles per row -- and at most kGradMaxRows rows:
// the pixel kernels carry the row on grid.y (a short spectrum's rows are ~2 KB each, so the byte bound alone would
// allow ~200 000 of them), the same cap as the likelihood's wide path (host_abi.cpp: wide_rows_per_pass).
constexpr int64_t kGradMaxRows = 65535;
// An HVP pass (`hvp`) also holds q, dq and the taps' second R derivative per row; the other entries' passes stay as they were.
int64_t grad_chunk_rows(const mcalf_ctx* ctx, bool hvp = false) {
    int64_t per_row = (2 * (int64_t)ctx->npix + 2 * (int64_t)grad_tapcap(ctx) + kGradRow +
                       (int64_t)grad_nslots(ctx) * kGradRec + (int64_t)grad_ntiles(ctx) * ctx->ndim) * (int64_t)sizeof(double);
    if (hvp) per_row += (2 * (int64_t)ctx->npix + (int64_t)grad_tapcap(ctx)) * (int64_t)sizeof(double);
    return std::min<int64_t>(kGradMaxRows, std::max<int64_t>(1, (int64_t)kGradChunkBytes / per_row));
}

// Everything a pass of `rows` rows needs, grown once (a later call of as many rows or fewer allocates nothing).  The VJP
// reads q from the caller's array and needs no q workspace (`own_q` false); its passes are cut as the gradient's all the same.
int grad_prepare(mcalf_ctx* ctx, int64_t batch, bool own_q = true) {
    const size_t rows = (size_t)std::min<int64_t>(batch, grad_chunk_rows(ctx));
    int rc;
    if ((rc = grow(ctx, &ctx->g_rows, &ctx->cap_g_rows, rows * kGradRow))) return rc;
    if ((rc = grow(ctx, &ctx->g_recs, &ctx->cap_g_recs, rows * grad_nslots(ctx) * kGradRec))) return rc;
    if ((rc = grow(ctx, &ctx->g_taps, &ctx->cap_g_taps, rows * grad_tapcap(ctx)))) return rc;
    if ((rc = grow(ctx, &ctx->g_dtaps, &ctx->cap_g_dtaps, rows * grad_tapcap(ctx)))) return rc;
    if ((rc = grow(ctx, &ctx->g_F, &ctx->cap_g_F, rows * ctx->npix))) return rc;
    if (own_q && (rc = grow(ctx, &ctx->g_q, &ctx->cap_g_q, rows * ctx->npix))) return rc;
    return grow(ctx, &ctx->g_part, &ctx->cap_g_part, rows * grad_ntiles(ctx) * ctx->ndim);
}

// The HVP's pass: the shared workspaces for its (smaller) row count, q, dq, the taps' second derivative, and logL of the batch.
int hvp_prepare(mcalf_ctx* ctx, int64_t batch) {
    const int64_t rows64 = std::min<int64_t>(batch, grad_chunk_rows(ctx, true));
    const size_t rows = (size_t)rows64;
    int rc;
    if ((rc = grad_prepare(ctx, rows64))) return rc;
    if ((rc = grow(ctx, &ctx->g_ddtaps, &ctx->cap_g_ddtaps, rows * grad_tapcap(ctx)))) return rc;
    if ((rc = grow(ctx, &ctx->g_hq, &ctx->cap_g_hq, rows * ctx->npix))) return rc;
    if ((rc = grow(ctx, &ctx->g_hdq, &ctx->cap_g_hdq, rows * ctx->npix))) return rc;
    return grow(ctx, &ctx->g_logL, &ctx->cap_g_logL, (size_t)batch);
}

// What every pass of a batch shares; the row pointers and the row count are set per pass.
GradArgs grad_args(const mcalf_ctx* ctx) {
    GradArgs a = {};
    a.nu = ctx->d_nu; a.obj = ctx->d_obj; a.ispec2 = ctx->d_ispec2; a.lgis = ctx->d_lgis; a.lines = ctx->d_lines;
    a.rows = ctx->g_rows; a.recs = ctx->g_recs; a.taps = ctx->g_taps; a.dtaps = ctx->g_dtaps;
    a.F = ctx->g_F; a.q = ctx->g_q; a.part = ctx->g_part;
    a.ddtaps = ctx->g_ddtaps; a.hq = ctx->g_hq; a.hdq = ctx->g_hdq;
    a.npix = (int)ctx->npix; a.ndim = ctx->ndim; a.ntiles = grad_ntiles(ctx); a.tapcap = grad_tapcap(ctx); a.nslots = grad_nslots(ctx);
    a.nlines = ctx->nlines; a.ncompmax = ctx->ncompmax; a.nfill = ctx->nfill; a.startind = ctx->startind; a.endind = ctx->endind;
    a.freespecres = ctx->freespecres; a.freecont = ctx->freecont; a.jax = ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX ? 1 : 0;
    a.jax_half = ctx->jax_half; a.n_cap = grad_ncap(ctx);
    a.specres_fixed = ctx->specres_fixed; a.contval_fixed = ctx->contval_fixed; a.velstep = ctx->velstep;
    return a;
}

// One kernel of a pass: every kernel takes the argument block by value.
int grad_kernel(mcalf_ctx* ctx, const void* fn, dim3 grid, const GradArgs& a, hipStream_t stream) {
    void* args[] = {(void*)&a};
    HIP_TRY(ctx, hipLaunchKernel(fn, grid, dim3(kGradBlock), args, 0, stream));
    return MCALF_OK;
}

// setup, forward, model, adjoint, deriv, finalize over the rows of `a`; `vjp`: the cotangent variants of model and finalize.
int grad_pass(mcalf_ctx* ctx, const GradArgs& a, bool vjp, hipStream_t stream) {
    const dim3 px((unsigned)a.ntiles, (unsigned)a.nrows);
    const int64_t cells = (int64_t)a.nrows * a.ndim;
    int rc;
    if ((rc = grad_kernel(ctx, grad_setup_kernel_ptr(), dim3((unsigned)a.nrows), a, stream))) return rc;
    if ((rc = grad_kernel(ctx, grad_forward_kernel_ptr(), px, a, stream))) return rc;
    if ((rc = grad_kernel(ctx, vjp ? vjp_model_kernel_ptr() : grad_model_kernel_ptr(), px, a, stream))) return rc;
    if ((rc = grad_kernel(ctx, grad_adjoint_kernel_ptr(), px, a, stream))) return rc;
    if ((rc = grad_kernel(ctx, grad_deriv_kernel_ptr(), px, a, stream))) return rc;
    return grad_kernel(ctx, vjp ? vjp_finalize_kernel_ptr() : grad_finalize_kernel_ptr(),
                       dim3((unsigned)((cells + kGradBlock - 1) / kGradBlock)), a, stream);
}

// logL of the batch (the likelihood's launch, which sizes its own workspaces -- per pass of rows on a wide-LSF context), then
// the gradient kernels pass by pass; all on `stream`.
int grad_launch(mcalf_ctx* ctx, const double* dP, int64_t batch, double* dlogL, double* dG, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    int rc = grad_prepare(ctx, batch);
    if (rc) return rc;
    if ((rc = launch(ctx, kModeLogL, dP, batch, 0, 0, dlogL, nullptr, stream))) return rc;
    GradArgs a = grad_args(ctx);
    const int64_t chunk = grad_chunk_rows(ctx);
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        a.P = dP + (size_t)row0 * ctx->ndim;
        a.logL = dlogL + row0;
        a.G = dG + (size_t)row0 * ctx->ndim;
        a.nrows = (int)std::min(chunk, batch - row0);
        if ((rc = grad_pass(ctx, a, false, stream))) return rc;
    }
    return MCALF_OK;
}

// dM = J(P) V row by row: setup, the tangent Voigt pass, the convolutions.
int jvp_launch(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* ddM, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    int rc = grad_prepare(ctx, batch);
    if (rc) return rc;
    GradArgs a = grad_args(ctx);
    const int64_t chunk = grad_chunk_rows(ctx);
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        a.P = dP + (size_t)row0 * ctx->ndim;
        a.V = dV + (size_t)row0 * ctx->ndim;
        a.dM = ddM + (size_t)row0 * ctx->npix;
        a.nrows = (int)std::min(chunk, batch - row0);
        const dim3 px((unsigned)a.ntiles, (unsigned)a.nrows);
        if ((rc = grad_kernel(ctx, grad_setup_kernel_ptr(), dim3((unsigned)a.nrows), a, stream))) return rc;
        if ((rc = grad_kernel(ctx, jvp_forward_kernel_ptr(), px, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, jvp_model_kernel_ptr(), px, a, stream))) return rc;
    }
    return MCALF_OK;
}

// G = J(P)^T Q row by row: the gradient's pass with the caller's cotangent rows as q (read only).
int vjp_launch(mcalf_ctx* ctx, const double* dP, const double* dQ, int64_t batch, double* dG, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    int rc = grad_prepare(ctx, batch, false);
    if (rc) return rc;
    GradArgs a = grad_args(ctx);
    const int64_t chunk = grad_chunk_rows(ctx);
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        a.P = dP + (size_t)row0 * ctx->ndim;
        a.q = const_cast<double*>(dQ) + (size_t)row0 * ctx->npix;
        a.G = dG + (size_t)row0 * ctx->ndim;
        a.nrows = (int)std::min(chunk, batch - row0);
        if ((rc = grad_pass(ctx, a, true, stream))) return rc;
    }
    return MCALF_OK;
}

// HV = (d2 logL / dtheta2)(P) V row by row.  logL of the batch (for the veto rule) comes from the likelihood's launch into the
// context's own g_logL; then per pass setup, the taps' second derivative, the tangent Voigt pass, q / dq, g / dg, the
// second-order Voigt pass and the gradient's finalize.
int hvp_launch(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dHV, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    int rc = hvp_prepare(ctx, batch);
    if (rc) return rc;
    if ((rc = launch(ctx, kModeLogL, dP, batch, 0, 0, ctx->g_logL, nullptr, stream))) return rc;
    GradArgs a = grad_args(ctx);
    const int64_t chunk = grad_chunk_rows(ctx, true);
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        a.P = dP + (size_t)row0 * ctx->ndim;
        a.V = dV + (size_t)row0 * ctx->ndim;
        a.logL = ctx->g_logL + row0;
        a.G = dHV + (size_t)row0 * ctx->ndim;
        a.nrows = (int)std::min(chunk, batch - row0);
        const dim3 px((unsigned)a.ntiles, (unsigned)a.nrows), row((unsigned)a.nrows);
        const int64_t cells = (int64_t)a.nrows * a.ndim;
        if ((rc = grad_kernel(ctx, grad_setup_kernel_ptr(), row, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, hvp_taps_kernel_ptr(), row, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, jvp_forward_kernel_ptr(), px, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, hvp_model_kernel_ptr(), px, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, hvp_adjoint_kernel_ptr(), px, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, hvp_deriv_kernel_ptr(), px, a, stream))) return rc;
        if ((rc = grad_kernel(ctx, grad_finalize_kernel_ptr(), dim3((unsigned)((cells + kGradBlock - 1) / kGradBlock)), a, stream)))
            return rc;
    }
    return MCALF_OK;
}

// The host-pointer JVP (X = V [batch, ndim], Y = dM [batch, npix]) or VJP (X = Q [batch, npix], Y = G [batch, ndim]):
// P and X to the device, the kernels, Y back, all on the context's stream; a multi-device context cuts the rows over
// its devices.  g_G holds the [batch, ndim] operand (V in, or G out), g_X the [batch, npix] one.
struct DerivShard { bool jvp; const double *P, *X; double* Y; int64_t xw, yw; int ndim; };

int deriv_host(mcalf_ctx* ctx, bool jvp, const double* P, const double* X, int64_t batch, double* Y) {
    if (!ctx || batch < 0 || (batch > 0 && (!P || !X || !Y))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (batch == 0) return MCALF_OK;
    const int64_t xw = jvp ? ctx->ndim : ctx->npix, yw = jvp ? ctx->npix : ctx->ndim;
    if (is_multi(ctx)) {                                  // contiguous row blocks, one per device, straight into the caller's arrays
        DerivShard c = {jvp, P, X, Y, xw, yw, ctx->ndim};
        return multi_run(ctx, batch, [](void* sub, int64_t lo, int64_t hi, void* arg) {
            const DerivShard* s = static_cast<const DerivShard*>(arg);
            return deriv_host(static_cast<mcalf_ctx*>(sub), s->jvp, s->P + (size_t)lo * s->ndim, s->X + (size_t)lo * s->xw, hi - lo,
                              s->Y + (size_t)lo * s->yw);
        }, &c);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)batch * ctx->ndim, pixels = (size_t)batch * ctx->npix;
    int rc;
    if ((rc = grow(ctx, &ctx->g_P, &ctx->cap_g_P, cells))) return rc;
    if ((rc = grow(ctx, &ctx->g_G, &ctx->cap_g_G, cells))) return rc;
    if ((rc = grow(ctx, &ctx->g_X, &ctx->cap_g_X, pixels))) return rc;
    double *dX = jvp ? ctx->g_G : ctx->g_X, *dY = jvp ? ctx->g_X : ctx->g_G;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->g_P, P, cells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dX, X, (size_t)batch * xw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = jvp ? jvp_launch(ctx, ctx->g_P, dX, batch, dY, ctx->stream) : vjp_launch(ctx, ctx->g_P, dX, batch, dY, ctx->stream)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(Y, dY, (size_t)batch * yw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->last.path = MCALF_PATH_HOST_STAGED;
    ctx->last.pinned_in = is_pinned_host(P) ? 1 : 0;
    ctx->last.pinned_out = is_pinned_host(Y) ? 1 : 0;
    return MCALF_OK;
}

int deriv_device(mcalf_ctx* ctx, bool jvp, const double* dP, const double* dX, int64_t batch, double* dY, void* stream) {
    if (!ctx || batch < 0 || (batch > 0 && (!dP || !dX || !dY))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, jvp ? "mcalf_model_jvp_batch_device" : "mcalf_model_vjp_batch_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->last.path = MCALF_PATH_DEVICE; ctx->last.pinned_in = ctx->last.pinned_out = 0;
    return jvp ? jvp_launch(ctx, dP, dX, batch, dY, (hipStream_t)stream) : vjp_launch(ctx, dP, dX, batch, dY, (hipStream_t)stream);
}

}  // namespace

void grad_release(mcalf_ctx* ctx) {
    double* bufs[] = {ctx->g_rows, ctx->g_recs, ctx->g_taps, ctx->g_dtaps, ctx->g_F, ctx->g_q, ctx->g_part, ctx->g_P, ctx->g_logL, ctx->g_G, ctx->g_X,
                      ctx->g_ddtaps, ctx->g_hq, ctx->g_hdq, ctx->g_V};
    for (double* b : bufs)
        if (b) (void)hipFree(b);
}

extern "C" int mcalf_loglike_grad_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, double* dlogL, double* dG,
                                               void* stream) {
    if (!ctx || batch < 0 || (batch > 0 && (!dP || !dlogL || !dG))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, "mcalf_loglike_grad_batch_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->last.path = MCALF_PATH_DEVICE; ctx->last.pinned_in = ctx->last.pinned_out = 0;
    return grad_launch(ctx, dP, batch, dlogL, dG, (hipStream_t)stream);
}

extern "C" int mcalf_loglike_grad_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* logL, double* G) {
    if (!ctx || batch < 0 || (batch > 0 && (!P || !G))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (batch == 0) return MCALF_OK;
    if (is_multi(ctx)) {                                  // contiguous row blocks, one per device, straight into the caller's arrays
        struct GradShard { const double* P; double *logL, *G; int ndim; } c = {P, logL, G, ctx->ndim};
        return multi_run(ctx, batch, [](void* sub, int64_t lo, int64_t hi, void* arg) {
            const GradShard* s = static_cast<const GradShard*>(arg);
            return mcalf_loglike_grad_batch(static_cast<mcalf_ctx*>(sub), s->P + (size_t)lo * s->ndim, hi - lo,
                                            s->logL ? s->logL + lo : nullptr, s->G + (size_t)lo * s->ndim);
        }, &c);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)batch * ctx->ndim;
    int rc;
    if ((rc = grow(ctx, &ctx->g_P, &ctx->cap_g_P, cells))) return rc;
    if ((rc = grow(ctx, &ctx->g_G, &ctx->cap_g_G, cells))) return rc;
    if ((rc = grow(ctx, &ctx->g_logL, &ctx->cap_g_logL, (size_t)batch))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->g_P, P, cells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = grad_launch(ctx, ctx->g_P, batch, ctx->g_logL, ctx->g_G, ctx->stream))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(G, ctx->g_G, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (logL) HIP_TRY(ctx, hipMemcpyAsync(logL, ctx->g_logL, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->last.path = MCALF_PATH_HOST_STAGED;              // H2D, launch, D2H on the context's stream (set after the launch's own)
    ctx->last.pinned_in = is_pinned_host(P) ? 1 : 0;
    ctx->last.pinned_out = is_pinned_host(G) ? 1 : 0;
    return MCALF_OK;
}

extern "C" int mcalf_model_jvp_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* dM) {
    return deriv_host(ctx, true, P, V, batch, dM);
}

extern "C" int mcalf_model_jvp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* ddM, void* stream) {
    return deriv_device(ctx, true, dP, dV, batch, ddM, stream);
}

extern "C" int mcalf_model_vjp_batch(mcalf_ctx* ctx, const double* P, const double* Q, int64_t batch, double* G) {
    return deriv_host(ctx, false, P, Q, batch, G);
}

extern "C" int mcalf_model_vjp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dQ, int64_t batch, double* dG, void* stream) {
    return deriv_device(ctx, false, dP, dQ, batch, dG, stream);
}

extern "C" int mcalf_loglike_hvp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dHV, void* stream) {
    if (!ctx || batch < 0 || (batch > 0 && (!dP || !dV || !dHV))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, "mcalf_loglike_hvp_batch_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->last.path = MCALF_PATH_DEVICE; ctx->last.pinned_in = ctx->last.pinned_out = 0;
    return hvp_launch(ctx, dP, dV, batch, dHV, (hipStream_t)stream);
}

extern "C" int mcalf_loglike_hvp_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* HV) {
    if (!ctx || batch < 0 || (batch > 0 && (!P || !V || !HV))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (batch == 0) return MCALF_OK;
    if (is_multi(ctx)) {                                  // contiguous row blocks, one per device, cut as the gradient's
        struct HvpShard { const double *P, *V; double* HV; int ndim; } c = {P, V, HV, ctx->ndim};
        return multi_run(ctx, batch, [](void* sub, int64_t lo, int64_t hi, void* arg) {
            const HvpShard* s = static_cast<const HvpShard*>(arg);
            return mcalf_loglike_hvp_batch(static_cast<mcalf_ctx*>(sub), s->P + (size_t)lo * s->ndim, s->V + (size_t)lo * s->ndim, hi - lo,
                                           s->HV + (size_t)lo * s->ndim);
        }, &c);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)batch * ctx->ndim;
    int rc;
    if ((rc = grow(ctx, &ctx->g_P, &ctx->cap_g_P, cells))) return rc;
    if ((rc = grow(ctx, &ctx->g_V, &ctx->cap_g_V, cells))) return rc;
    if ((rc = grow(ctx, &ctx->g_G, &ctx->cap_g_G, cells))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->g_P, P, cells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->g_V, V, cells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = hvp_launch(ctx, ctx->g_P, ctx->g_V, batch, ctx->g_G, ctx->stream))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(HV, ctx->g_G, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->last.path = MCALF_PATH_HOST_STAGED;
    ctx->last.pinned_in = is_pinned_host(P) ? 1 : 0;
    ctx->last.pinned_out = is_pinned_host(HV) ? 1 : 0;
    return MCALF_OK;
}

extern "C" int mcalf_voigt_hjerting_grad(const double* x, const double* y, int64_t n, double* out, int32_t device) {
    if (n < 0 || (n > 0 && (!x || !y || !out))) return set_err(nullptr, MCALF_ERR_INVALID, "bad arguments");
    if (n == 0) return MCALF_OK;
    int dev = 0;
    int rc = pick_device(nullptr, device, &dev, nullptr);
    if (rc) return rc;
    HIP_TRY(nullptr, hipSetDevice(dev));
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    hipError_t e = hipMalloc((void**)&dx, nb);
    if (e == hipSuccess) e = hipMalloc((void**)&dy, nb);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, 3 * nb);
    if (e == hipSuccess) e = hipMemcpy(dx, x, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, y, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        long cnt = (long)n;
        void* kargs[] = {(void*)&dx, (void*)&dy, (void*)&cnt, (void*)&dout};
        e = hipLaunchKernel(grad_hjert_kernel_ptr(), dim3((unsigned)((n + 255) / 256)), dim3(256), kargs, 0, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, 3 * nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(nullptr, MCALF_ERR_HIP, "hjerting_grad: %s", hipGetErrorString(e));
    for (double* b : {dx, dy, dout})
        if (b) (void)hipFree(b);
    return rc;
}
