// What the fit kernels (fit_kernels.hip) and their host side (host_fit.cpp) share: the argument block, the workspace layout
// and the kernel handles.  Plain C++ -- host_fit.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"
#include "theta_row.h"

namespace mcalf {

constexpr int kFitWave = 64;             // threads per workgroup of the row kernels: ONE wave per row, lane k owns parameters k, k + 64, ...
constexpr int kFitPixBlock = 256;        // threads per workgroup of the weight kernel, one pixel per thread
constexpr int kFitScal = 4;              // per-row scalars in `scal`: [0][rows] lambda, [1][rows] r.r, [2][rows] g.g, [3][rows] logL of the trial
constexpr double kFitCgTol = 1e-20;      // a row's CG freezes when r.r <= kFitCgTol g.g
constexpr double kFitLambdaMin = 1e-15, kFitLambdaMax = 1e12;

// Status of a row.  0 while it is live (and at the end: max_iter reached).
enum { kFitLive = 0, kFitConverged = 1, kFitZeroGrad = 2, kFitLambdaOut = 3, kFitBadStart = -1 };

// One row block of a fit (rows [row0, row0 + nrows) of the caller's arrays); the weight kernel reads dM, W, nrows, npix only.
struct FitArgs {
    const double* P0;         // the caller's starts [nrows, ndim] (read by the start kernels only)
    double* th;               // the current point, the caller's P rows [nrows, ndim]
    double* L;                // its logL, the caller's logL rows [nrows]
    int32_t *status, *niter;  // the caller's rows [nrows]
    const double *lo, *hi;    // the prior box [ndim] each
    double *T, *G, *GT;       // trial point, gradient at th, gradient at T           [nrows, ndim]
    double *gu, *x, *r, *p;   // cube-unit gradient with the pins zeroed, CG iterate, residual, direction
    double* V;                // s (.) p, the tangent of the next Fisher product
    const double* FV;         // J^T W J V, its result
    double* scal;             // per-row scalars [kFitScal][nrows]
    int32_t* frozen;          // [nrows] the row's CG has stopped for this outer iteration
    int32_t* pin;             // [nrows, ndim] 1: the coordinate does not move in this outer iteration
    unsigned int* live;       // rows still live after the accept kernel (integer counter)
    double* dM;               // weight kernel: [nrows, npix], dM <- W (.) dM
    const double* W;          // [npix]
    int nrows, npix;
    double lambda0, ftol;
    RowLayout lay;            // how a row is read (theta_row.h); the weight kernel does not look at it
};

// The kernels of fit_kernels.hip; all take (const FitArgs a).
enum FitKernel {
    // grid = nrows, kFitWave threads: one wave per row
    kFitStart,        // th = P0 with the continuous, active entries clamped into the box; lambda0, status 0, niter 0
    kFitStarted,      // after the gradient at th: a start whose logL is not finite is status -1 and returned as given
    kFitBegin,        // pins, g_u, x = 0, r = p = g_u, r.r, g.g, V = s (.) p; all-zero g_u is status 2
    kFitCg,           // one CG update from FV; V for the next product
    kFitTrial,        // T = clamp(th + s (.) x)
    kFitAccept,       // accept / reject, lambda, status, the live counter
    // grid = (ceil(npix / kFitPixBlock), nrows), kFitPixBlock threads
    kFitWeight,       // dM <- W (.) dM
    kFitKernelCount
};
MCALF_INTERNAL const void* fit_kernel_ptr(FitKernel k);

}  // namespace mcalf
