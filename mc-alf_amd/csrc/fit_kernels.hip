// Device side of the batched Levenberg-Marquardt fit (mcalf_maximize_batch) and of the Fisher product
// (mcalf_fisher_matvec_batch), for gfx950.  The Voigt work -- logL, its gradient, J v and J^T q -- is the derivative kernels'
// (grad_kernels.hip, issued by host_fit.cpp through host_grad.cpp's products); what lives here is the per-row linear algebra
// that keeps the loop on the device, and the per-pixel weight of the Fisher product.
//
//   weight    one pixel per thread: dM <- W (.) dM, ONE IEEE multiply per pixel.
//   the rest  ONE wave64 per row, lane k owns parameters k, k + 64, ... (any ndim).  A dot product: every lane adds its own
//             entries in index order, the 64 lane sums go through one fixed xor-butterfly (every lane ends with the same
//             bits), and the row's scalars are made wave-uniform with readfirstlane.
// No floating-point atomics (the counter of live rows is an integer) and one summation order: a row's bits depend on its
// own start alone -- not on its batch, its position or the row block it falls in.  A finished row (status != 0) is carried:
// every kernel leaves its point, its logL and its gradient as they are.
#include <hip/hip_runtime.h>

#include "fit_args.h"
#include "wave_row.h"

using namespace mcalf;

namespace {

__device__ __forceinline__ double clamp_keep_nan(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

__global__ __launch_bounds__(kFitWave) void mcalf_fit_start_kernel(const FitArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const double* p0 = a.P0 + (size_t)row * a.lay.ndim;
    double* th = a.th + (size_t)row * a.lay.ndim;
    const int nc = active_components(a.lay, p0[a.lay.startind]);
    for (int k = lane; k < a.lay.ndim; k += kFitWave) {
        const double v = p0[k];
        th[k] = coord_movable(a.lay, nc, k) ? clamp_keep_nan(v, a.lo[k], a.hi[k]) : v;
    }
    if (lane == 0) {
        a.scal[row] = a.lambda0;
        a.status[row] = kFitLive;
        a.niter[row] = 0;
        a.frozen[row] = 0;
    }
}

// A start is bad when its logL is not finite or when one of its continuous, active entries is NaN (np.nansum drops every
// pixel of such a row: its logL is a finite 0 that says nothing).
__global__ __launch_bounds__(kFitWave) void mcalf_fit_started_kernel(const FitArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const double* p0 = a.P0 + (size_t)row * a.lay.ndim;
    double* th = a.th + (size_t)row * a.lay.ndim;
    const int nc = active_components(a.lay, p0[a.lay.startind]);
    int nan = 0;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) nan |= (coord_movable(a.lay, nc, k) && isnan(p0[k])) ? 1 : 0;
    if (isfinite(a.L[row]) && !__any(nan)) return;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) th[k] = p0[k];
    if (lane == 0) a.status[row] = kFitBadStart;
}

__global__ __launch_bounds__(kFitWave) void mcalf_fit_begin_kernel(const FitArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)row * a.lay.ndim;
    double* V = a.V + o;
    if (__builtin_amdgcn_readfirstlane(a.status[row]) != kFitLive) {
        for (int k = lane; k < a.lay.ndim; k += kFitWave) V[k] = 0.0;
        return;
    }
    const double *th = a.th + o, *G = a.G + o;
    const int nc = active_components(a.lay, th[a.lay.startind]);
    double part = 0.0;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) {
        const double lo = a.lo[k], hi = a.hi[k], s = hi - lo, t = th[k], g = G[k];
        const bool pinned = !coord_movable(a.lay, nc, k) || !(s > 0.0) || (t <= lo && g < 0.0) || (t >= hi && g > 0.0);
        const double gk = pinned ? 0.0 : s * g;
        a.pin[o + k] = pinned ? 1 : 0;
        a.gu[o + k] = gk;
        a.x[o + k] = 0.0;
        a.r[o + k] = gk;
        a.p[o + k] = gk;
        V[k] = pinned ? 0.0 : s * gk;
        part += gk * gk;
    }
    const double gg = uniform(wave_sum(part));
    if (lane != 0) return;
    if (!(gg > 0.0)) {
        a.status[row] = kFitZeroGrad;
        return;
    }
    a.niter[row] += 1;
    a.frozen[row] = 0;
    a.scal[(size_t)a.nrows + row] = gg;
    a.scal[2 * (size_t)a.nrows + row] = gg;
}

// One conjugate-gradient update of (A + lambda I) x = g_u with A p = s (.) FV on the unpinned coordinates.  A p is kept in T
// (the trial kernel writes T only after the last update).
__global__ __launch_bounds__(kFitWave) void mcalf_fit_cg_kernel(const FitArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (__builtin_amdgcn_readfirstlane(a.status[row]) != kFitLive || __builtin_amdgcn_readfirstlane(a.frozen[row])) return;
    const size_t o = (size_t)row * a.lay.ndim;
    const double lam = a.scal[row], rr = a.scal[(size_t)a.nrows + row], gg = a.scal[2 * (size_t)a.nrows + row];
    double* Ap = a.T + o;
    double part = 0.0;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) {
        const double pk = a.p[o + k];
        const double ap = a.pin[o + k] ? 0.0 : (a.hi[k] - a.lo[k]) * a.FV[o + k] + lam * pk;
        Ap[k] = ap;
        part += pk * ap;
    }
    const double pAp = uniform(wave_sum(part));
    if (!(pAp > 0.0)) {
        if (lane == 0) a.frozen[row] = 1;
        return;
    }
    const double alpha = rr / pAp;
    part = 0.0;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) {
        a.x[o + k] += alpha * a.p[o + k];
        const double rk = a.r[o + k] - alpha * Ap[k];
        a.r[o + k] = rk;
        part += rk * rk;
    }
    const double rrn = uniform(wave_sum(part));
    if (lane == 0) a.scal[(size_t)a.nrows + row] = rrn;
    if (rrn <= kFitCgTol * gg) {
        if (lane == 0) a.frozen[row] = 1;
        return;
    }
    const double beta = rrn / rr;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) {
        const double pk = a.r[o + k] + beta * a.p[o + k];
        a.p[o + k] = pk;
        a.V[o + k] = a.pin[o + k] ? 0.0 : (a.hi[k] - a.lo[k]) * pk;
    }
}

__global__ __launch_bounds__(kFitWave) void mcalf_fit_trial_kernel(const FitArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)row * a.lay.ndim;
    const bool live = __builtin_amdgcn_readfirstlane(a.status[row]) == kFitLive;
    for (int k = lane; k < a.lay.ndim; k += kFitWave) {
        const double t = a.th[o + k];
        double v = t;
        if (live && !a.pin[o + k]) v = clamp_keep_nan(t + (a.hi[k] - a.lo[k]) * a.x[o + k], a.lo[k], a.hi[k]);
        a.T[o + k] = v;
    }
}

__global__ __launch_bounds__(kFitWave) void mcalf_fit_accept_kernel(const FitArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (__builtin_amdgcn_readfirstlane(a.status[row]) != kFitLive) return;
    const size_t o = (size_t)row * a.lay.ndim;
    const double l0 = a.L[row], l1 = a.scal[3 * (size_t)a.nrows + row], lam = a.scal[row];
    int st = kFitLive;
    double lamn;
    if (isfinite(l1) && l1 > l0) {
        for (int k = lane; k < a.lay.ndim; k += kFitWave) {
            a.th[o + k] = a.T[o + k];
            a.G[o + k] = a.GT[o + k];
        }
        lamn = fmax(lam / 10.0, kFitLambdaMin);
        if (l1 - l0 <= a.ftol * (1.0 + fabs(l1))) st = kFitConverged;
        if (lane == 0) a.L[row] = l1;
    } else {
        lamn = 10.0 * lam;
        if (lamn > kFitLambdaMax) st = kFitLambdaOut;
    }
    if (lane != 0) return;
    a.scal[row] = lamn;
    if (st != kFitLive) a.status[row] = st;
    else atomicAdd(a.live, 1u);
}

__global__ __launch_bounds__(kFitPixBlock) void mcalf_fit_weight_kernel(const FitArgs a) {
    const int i = blockIdx.x * kFitPixBlock + threadIdx.x;
    if (i >= a.npix) return;
    double* d = a.dM + (size_t)blockIdx.y * a.npix + i;
    *d = a.W[i] * *d;
}

namespace mcalf {
const void* fit_kernel_ptr(FitKernel k) {
    static const void* const table[] = {(const void*)&mcalf_fit_start_kernel, (const void*)&mcalf_fit_started_kernel,
                                        (const void*)&mcalf_fit_begin_kernel, (const void*)&mcalf_fit_cg_kernel,
                                        (const void*)&mcalf_fit_trial_kernel, (const void*)&mcalf_fit_accept_kernel,
                                        (const void*)&mcalf_fit_weight_kernel};   // in the order of enum FitKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kFitKernelCount, "one entry per FitKernel");
    return table[k];
}
}  // namespace mcalf
