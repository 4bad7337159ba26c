// What the derivative kernels (grad_kernels.hip) and their host side (host_grad.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_grad.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"
#include "theta_row.h"

namespace mcalf {

constexpr int kGradBlock = 256;          // threads per workgroup; one pixel per thread, so also the tile of the pixel kernels
constexpr int kGradRec = 6;              // doubles per (component, line) record: A, B, a, K, 1/dnu, 1/b
constexpr int kGradRow = 8;              // doubles per row: R, cont, half-width n, active components, bad flag, bot, (pad)
constexpr size_t kGradChunkBytes = size_t(384) << 20;   // per-row workspaces of one pass (F, q, taps, ...) at most this big

// One pass over `nrows` rows of a batch (rows [row0, row0 + nrows) of the caller's arrays).
struct GradArgs {
    const double* P;          // parameter rows of this pass, row-major [nrows, ndim]
    const double* logL;       // their logL (the fused kernel's): -inf / NaN rows get an all-NaN gradient
    double* G;                // gradient rows of this pass [nrows, ndim]
    const double *nu, *obj, *ispec2, *lgis;
    const LineDev* lines;     // nlines target lines, then the filler line
    double *rows, *recs, *taps, *dtaps;      // per-row workspaces: [nrows, kGradRow], [nrows, nslots, kGradRec], [nrows, tapcap] x 2
    double *F, *q;            // [nrows, npix]: transmitted flux (then g = -F cont L^T q), weighted residual
    double* part;             // [nrows, ntiles, ndim] per-tile partial sums of the gradient
    int nrows, npix, ntiles, tapcap, nslots, jax_half, n_cap;
    double velstep;
    RowLayout lay;            // how a row of P is read (theta_row.h)
    // The JVP and the HVP keep T = dF in `q`; the VJP points `q` at the caller's cotangent rows, which no kernel of its pass writes.
    const double* V;          // JVP, HVP: tangent rows of this pass [nrows, ndim]
    double* dM;               // JVP: directional derivative of the model [nrows, npix]
    double* ddtaps;           // HVP: d2 w_k / dR2 of the normalised taps [nrows, tapcap]
    double *hq, *hdq;         // HVP: q = W (d - m) and dq = -W dM [nrows, npix] (F and q hold g and dg after its adjoint kernel)
};

// The kernels of grad_kernels.hip.  All but the last take (const GradArgs a) and kGradBlock threads per workgroup; the enum is
// ordered by grid, which host_grad.cpp derives from the handle alone.
enum GradKernel {
    // grid = nrows: one workgroup per row
    kGradSetup,          // decode, (component, line) records, normalised taps and their R derivative
    kGradHvpTaps,        // d2 w_k / dR2 of the taps the setup kernel left
    // grid = (ntiles, nrows): one pixel per thread
    kGradFirstPixel,
    kGradForward = kGradFirstPixel,   // F = exp(-tau)
    kGradModel,          // q = w (d - m); continuum and R partials
    kGradVjpModel,       // the model kernel with q = the caller's cotangent
    kGradAdjoint,        // g = -F cont L^T q (in place of F)
    kGradDeriv,          // (N, z, b) partials
    kGradJvpForward,     // F = exp(-tau), T = -F dtau along the row's tangent (in q)
    kGradJvpModel,       // dM = cont L(T) + v_cont L(F) + v_R cont (dL/dR)(F)
    kGradHvpModel,       // q, dq (hq, hdq); continuum and R partials of H v
    kGradHvpAdjoint,     // g and dg (in place of F and T)
    kGradHvpDeriv,       // (N, z, b) partials of H v, the second-order Voigt pass
    // grid = ceil(nrows * ndim / kGradBlock): one cell of G per thread
    kGradFirstCell,
    kGradFinalize = kGradFirstCell,   // tiles summed in order; -inf / NaN logL rows and rows beyond the tap cap get NaN
    kGradVjpFinalize,    // as finalize, without the logL veto rule
    // (const double* x, const double* y, long n, double* out), 256 threads per point block: out[3i..] = H, H_x, H_y
    kGradHjert,
    kGradKernelCount
};
MCALF_INTERNAL const void* grad_kernel_ptr(GradKernel k);

}  // namespace mcalf
