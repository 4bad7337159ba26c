// Host side of the derivative kernels (grad_kernels.hip): the analytic gradient of logL, the model Jacobian's JVP and VJP,
// the Hessian-vector product of logL, and mcalf_voigt_hjerting_grad.  A product is a row of the table below -- its
// workspaces, whether logL comes first, its kernel sequence, its row pointers -- and ONE driver (run_product) runs any of
// them pass by pass over row blocks whose per-row workspaces stay within kGradChunkBytes.  logL itself comes from the
// likelihood's own launch (host_launch.cpp: launch), so the entries agree on it bit for bit.  ONE helper serves the
// host-pointer entries (run_host: the staged call of host_staged.cpp) and one the device-pointer entries (run_device).
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

// Doubles per row of per-row workspace `b` (one of ctx->gb[0, kGbHvp)).
int64_t ws_row_elems(const mcalf_ctx* ctx, int b) {
    switch (b) {
        case mcalf_ctx::kGbRows: return kGradRow;
        case mcalf_ctx::kGbRecs: return (int64_t)grad_nslots(ctx) * kGradRec;
        case mcalf_ctx::kGbPart: return (int64_t)grad_ntiles(ctx) * ctx->ndim;
        case mcalf_ctx::kGbTaps: case mcalf_ctx::kGbDtaps: case mcalf_ctx::kGbDdtaps: return grad_tapcap(ctx);
        default: return ctx->npix;                                                  // F, q, hq, hdq
    }
}

// Rows per pass of a product whose per-row workspaces are ctx->gb[0, nws): EVERY one of them within kGradChunkBytes -- the
// taps of a wide-LSF context are thousands of doubles per row -- and at most kGradMaxRows rows: the pixel kernels carry the
// row on grid.y (a short spectrum's rows are ~2 KB each, so the byte bound alone would allow ~200 000 of them), the same cap
// as the likelihood's wide path (host_wide.cpp: wide_rows_per_pass).  The HVP's three more workspaces cut its passes smaller.
constexpr int64_t kGradMaxRows = 65535;
int64_t grad_chunk_rows(const mcalf_ctx* ctx, int nws) {
    int64_t per_row = 0;
    for (int b = 0; b < nws; ++b) per_row += ws_row_elems(ctx, b) * (int64_t)sizeof(double);
    return std::min<int64_t>(kGradMaxRows, std::max<int64_t>(1, (int64_t)kGradChunkBytes / per_row));
}

int grow_buf(mcalf_ctx* ctx, int b, size_t elems) { return grow(ctx, ctx->gb[b], elems); }

// What every pass of a batch shares; the row pointers and the row count are set per pass.
GradArgs grad_args(const mcalf_ctx* ctx) {
    GradArgs a = {};
    const DevBuf<double>* gb = ctx->gb;
    a.nu = ctx->d_nu; a.obj = ctx->d_obj; a.ispec2 = ctx->d_ispec2; a.lgis = ctx->d_lgis; a.lines = ctx->d_lines;
    a.rows = gb[mcalf_ctx::kGbRows]; a.recs = gb[mcalf_ctx::kGbRecs]; a.taps = gb[mcalf_ctx::kGbTaps]; a.dtaps = gb[mcalf_ctx::kGbDtaps];
    a.F = gb[mcalf_ctx::kGbF]; a.q = gb[mcalf_ctx::kGbQ]; a.part = gb[mcalf_ctx::kGbPart];
    a.ddtaps = gb[mcalf_ctx::kGbDdtaps]; a.hq = gb[mcalf_ctx::kGbHq]; a.hdq = gb[mcalf_ctx::kGbHdq];
    a.npix = (int)ctx->npix; a.ntiles = grad_ntiles(ctx); a.tapcap = grad_tapcap(ctx); a.nslots = grad_nslots(ctx);
    a.jax_half = ctx->jax_half; a.n_cap = grad_ncap(ctx); a.velstep = ctx->velstep;
    a.lay = row_layout(ctx);
    return a;
}

}  // namespace

// (struct Call and struct Product: host_ctx.h -- host_fit.cpp runs these products too)
extern const Product kProdGrad = {"mcalf_loglike_grad_batch_device", mcalf_ctx::kGbShared, true, true, true, false, false, false,
    {kGradSetup, kGradForward, kGradModel, kGradAdjoint, kGradDeriv, kGradFinalize, kGradKernelCount},
    [](GradArgs& a, const Call& c, size_t cell0, size_t, int64_t row0) { a.logL = c.L + row0; a.G = c.Y + cell0; }};
// dM = J(P) V row by row: setup, the tangent Voigt pass, the convolutions.
extern const Product kProdJvp = {"mcalf_model_jvp_batch_device", mcalf_ctx::kGbShared, true, false, false, true, false, true,
    {kGradSetup, kGradJvpForward, kGradJvpModel, kGradKernelCount},
    [](GradArgs& a, const Call& c, size_t cell0, size_t pix0, int64_t) { a.V = c.X + cell0; a.dM = c.Y + pix0; }};
// G = J(P)^T Q row by row: the gradient's pass with the caller's cotangent rows as q (read only) and no logL.
extern const Product kProdVjp = {"mcalf_model_vjp_batch_device", mcalf_ctx::kGbShared, false, false, false, true, true, false,
    {kGradSetup, kGradForward, kGradVjpModel, kGradAdjoint, kGradDeriv, kGradVjpFinalize, kGradKernelCount},
    [](GradArgs& a, const Call& c, size_t cell0, size_t pix0, int64_t) { a.q = const_cast<double*>(c.X) + pix0; a.G = c.Y + cell0; }};
// HV = (d2 logL / dtheta2)(P) V row by row: the taps' second derivative, the tangent Voigt pass, q / dq, g / dg, the
// second-order Voigt pass and the gradient's finalize (logL, for its veto rule, stays in the context's buffer).
extern const Product kProdHvp = {"mcalf_loglike_hvp_batch_device", mcalf_ctx::kGbHvp, true, true, false, true, false, false,
    {kGradSetup, kGradHvpTaps, kGradJvpForward, kGradHvpModel, kGradHvpAdjoint, kGradHvpDeriv, kGradFinalize, kGradKernelCount},
    [](GradArgs& a, const Call& c, size_t cell0, size_t, int64_t row0) { a.V = c.X + cell0; a.logL = c.L + row0; a.G = c.Y + cell0; }};

namespace {

dim3 grad_grid(GradKernel k, const GradArgs& a) {
    if (k < kGradFirstPixel) return dim3((unsigned)a.nrows);
    if (k < kGradFirstCell) return dim3((unsigned)a.ntiles, (unsigned)a.nrows);
    return dim3((unsigned)(((int64_t)a.nrows * a.lay.ndim + kGradBlock - 1) / kGradBlock));
}

}  // namespace

// Product `p` over a batch, all on `stream`: its workspaces for one pass (grown once: a later call of as many rows or fewer
// allocates nothing), logL of the batch where it needs one (the likelihood's launch, which sizes its own workspaces), then
// its kernels pass by pass; every kernel takes the argument block by value.
int run_product(mcalf_ctx* ctx, const Product& p, Call c, int64_t batch, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    const int64_t chunk = grad_chunk_rows(ctx, p.nws);
    const size_t rows = (size_t)std::min(batch, chunk);
    int rc;
    for (int b = 0; b < p.nws; ++b)
        if ((b != mcalf_ctx::kGbQ || p.own_q) && (rc = grow_buf(ctx, b, rows * (size_t)ws_row_elems(ctx, b)))) return rc;
    if (p.logl) {
        if (!c.L) {
            if ((rc = grow_buf(ctx, mcalf_ctx::kGbLogL, (size_t)batch))) return rc;
            c.L = ctx->gb[mcalf_ctx::kGbLogL];
        }
        LaunchReq q(kModeLogL, c.P, batch, stream); q.d_out = c.L;
        if ((rc = launch(ctx, q))) return rc;
    }
    GradArgs a = grad_args(ctx);
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        a.P = c.P + (size_t)row0 * ctx->ndim;
        a.nrows = (int)std::min(chunk, batch - row0);
        p.bind(a, c, (size_t)row0 * ctx->ndim, (size_t)row0 * ctx->npix, row0);
        for (const GradKernel* k = p.seq; *k != kGradKernelCount; ++k)
            if ((rc = LAUNCH_BLOCK(ctx, grad_kernel_ptr(*k), a, grad_grid(*k, a), dim3(kGradBlock), stream))) return rc;
    }
    return MCALF_OK;
}

int theta_logl_grad(mcalf_ctx* ctx, const double* P, double* L, double* G, int64_t n, hipStream_t stream) {
    return run_product(ctx, kProdGrad, {P, nullptr, G, L}, n, stream);
}

namespace {

int run_device(mcalf_ctx* ctx, const Product& p, const Call& c, int64_t batch, void* stream) {
    if (!ctx || batch < 0 || (batch > 0 && (!c.P || !c.Y || (p.has_x && !c.X) || (p.l_out && !c.L))))
        return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, p.device_entry);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_product(ctx, p, c, batch, (hipStream_t)stream);
}

// A host-pointer entry: P and X to the device, the product, Y (and logL where the caller wants it: L may be NULL) back -- the
// staged call of host_staged.cpp, rows cut over the devices.  logL comes from the product's own buffer.
enum { kColP, kColX, kColY, kColL };

int host_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    const int rc = run_product(ctx, *static_cast<const Product*>(arg), {(const double*)dev[kColP], (const double*)dev[kColX], (double*)dev[kColY], nullptr},
                               rows, stream);
    dev[kColL] = ctx->gb[mcalf_ctx::kGbLogL];
    return rc;
}

int run_host(mcalf_ctx* ctx, const Product& p, const double* P, const double* X, int64_t batch, double* Y, double* L) {
    if (!ctx || batch < 0 || (batch > 0 && (!P || !Y || (p.has_x && !X)))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (batch == 0) return MCALF_OK;
    const size_t d = sizeof(double), ndim = (size_t)ctx->ndim, npix = (size_t)ctx->npix;
    StagePlan plan = {{stage_in(P, d, ndim), stage_in(p.has_x ? X : nullptr, d, p.x_pix ? npix : ndim), stage_out(Y, d, p.y_pix ? npix : ndim),
                       stage_out(L, d, 1, true, true)}, 4, batch, kStageCutRows, kColP, kColY, host_body, const_cast<Product*>(&p)};
    return run_staged(ctx, plan);
}

}  // namespace

extern "C" int mcalf_loglike_grad_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, double* dlogL, double* dG,
                                               void* stream) {
    return run_device(ctx, kProdGrad, {dP, nullptr, dG, dlogL}, batch, stream);
}

extern "C" int mcalf_loglike_grad_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* logL, double* G) {
    return run_host(ctx, kProdGrad, P, nullptr, batch, G, logL);
}

extern "C" int mcalf_model_jvp_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* dM) {
    return run_host(ctx, kProdJvp, P, V, batch, dM, nullptr);
}

extern "C" int mcalf_model_jvp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* ddM, void* stream) {
    return run_device(ctx, kProdJvp, {dP, dV, ddM, nullptr}, batch, stream);
}

extern "C" int mcalf_model_vjp_batch(mcalf_ctx* ctx, const double* P, const double* Q, int64_t batch, double* G) {
    return run_host(ctx, kProdVjp, P, Q, batch, G, nullptr);
}

extern "C" int mcalf_model_vjp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dQ, int64_t batch, double* dG, void* stream) {
    return run_device(ctx, kProdVjp, {dP, dQ, dG, nullptr}, batch, stream);
}

extern "C" int mcalf_loglike_hvp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dHV, void* stream) {
    return run_device(ctx, kProdHvp, {dP, dV, dHV, nullptr}, batch, stream);
}

extern "C" int mcalf_loglike_hvp_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* HV) {
    return run_host(ctx, kProdHvp, P, V, batch, HV, nullptr);
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
        e = hipLaunchKernel(grad_kernel_ptr(kGradHjert), dim3((unsigned)((n + 255) / 256)), dim3(256), kargs, 0, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, 3 * nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(nullptr, MCALF_ERR_HIP, "hjerting_grad: %s", hipGetErrorString(e));
    for (double* b : {dx, dy, dout})
        if (b) (void)hipFree(b);
    return rc;
}
