// What the gradient, Jacobian-product and Hessian-product kernels (grad_kernels.hip) and their host side (host_grad.cpp) share: the argument block, the
// workspace layout and the kernel entry points.  Plain C++ -- host_grad.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"

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
    int nrows, npix, ndim, ntiles, tapcap, nslots;
    int nlines, ncompmax, nfill, startind, endind, freespecres, freecont, jax, jax_half, n_cap;
    double specres_fixed, contval_fixed, velstep;
    // the model Jacobian's products (appended: the gradient kernels' argument offsets stay as they were).  The JVP keeps
    // T = -F dtau in `q`; the VJP points `q` at the caller's cotangent rows, which no kernel of its pass writes.
    const double* V;          // JVP: tangent rows of this pass [nrows, ndim]
    double* dM;               // JVP: directional derivative of the model [nrows, npix]
    // the Hessian-vector product of logL (appended likewise).  Its pass keeps F and T = dF in `F` / `q` (jvp_forward), then
    // g and dg in their place; the weighted residual and its tangent need two workspaces of their own.
    double* ddtaps;           // HVP: d2 w_k / dR2 of the normalised taps [nrows, tapcap]
    double *hq, *hdq;         // HVP: q = W (d - m) and dq = -W dM [nrows, npix]
};

// grad_kernels.hip; every kernel takes (const GradArgs a), grid as stated
MCALF_INTERNAL const void* grad_setup_kernel_ptr();      // grid = nrows: decode, records, taps
MCALF_INTERNAL const void* grad_forward_kernel_ptr();    // grid = (ntiles, nrows): F = exp(-tau)
MCALF_INTERNAL const void* grad_model_kernel_ptr();      // grid = (ntiles, nrows): q, continuum and R partials
MCALF_INTERNAL const void* grad_adjoint_kernel_ptr();    // grid = (ntiles, nrows): g = -F cont L^T q (in place of F)
MCALF_INTERNAL const void* grad_deriv_kernel_ptr();      // grid = (ntiles, nrows): (N, z, b) partials
MCALF_INTERNAL const void* grad_finalize_kernel_ptr();   // grid = ceil(nrows * ndim / kGradBlock): tiles summed in order
MCALF_INTERNAL const void* vjp_model_kernel_ptr();       // grid = (ntiles, nrows): the model kernel with q = the caller's cotangent
MCALF_INTERNAL const void* vjp_finalize_kernel_ptr();    // as finalize, without the logL veto rule
MCALF_INTERNAL const void* jvp_forward_kernel_ptr();     // grid = (ntiles, nrows): F = exp(-tau), T = -F dtau along the row's tangent
MCALF_INTERNAL const void* jvp_model_kernel_ptr();       // grid = (ntiles, nrows): dM = cont L(T) + v_cont L(F) + v_R cont (dL/dR)(F)
MCALF_INTERNAL const void* hvp_taps_kernel_ptr();        // grid = nrows: d2 w_k / dR2 of the taps the setup kernel left
MCALF_INTERNAL const void* hvp_model_kernel_ptr();       // grid = (ntiles, nrows): q, dq; continuum and R partials of H v
MCALF_INTERNAL const void* hvp_adjoint_kernel_ptr();     // grid = (ntiles, nrows): g and dg (in place of F and T)
MCALF_INTERNAL const void* hvp_deriv_kernel_ptr();       // grid = (ntiles, nrows): (N, z, b) partials of H v, second-order Voigt pass
MCALF_INTERNAL const void* grad_hjert_kernel_ptr();      // (const double* x, const double* y, long n, double* out): out[3i..] = H, H_x, H_y

}  // namespace mcalf
