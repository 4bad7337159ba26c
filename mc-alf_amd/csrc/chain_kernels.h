// The chain-diagnostics kernels for gfx950, float64 (mcalf_chain_stats, mcalf_ensemble_converge): per coordinate of a chain
// X [T][n][d] the pooled mean and variance, the walker-averaged integrated autocorrelation time with Sokal's window, the same of
// the ensemble-mean series, split R-hat and the effective sample size.  The definitions, operation for operation, are in
// include/mcalf_hip.h; the argument block and the tile constants in chain_args.h.  Compiled as part of ens_kernels.hip's
// translation unit (its last line includes this file), under that file's `fp contract(off)`: every product and sum below is
// separately rounded but for the explicit fma of the autocovariance sums.  NOT a stand-alone header: it defines kernels and
// a kernel table, opens namespace mcalf at file scope and relies on the includer's pragma; nothing else may include it.
//
//   sums         one thread per (w, k), t ascending: S_w = sum x_t, delta_w = (sum (x_t - x_0)) / T, the means of the first and last
//                h = T / 2 states; a series with x_t == x_0 for every t is CONSTANT and has its half means = x_0 (a rounded sum of T
//                copies of 0.3 over T is not 0.3) and c_w(0) = 0 exactly, and it is left out.  The centred value of the ACF is
//                (x_t - x_0) - delta_w: x_t - x_0 is exact for values within a factor of two of each other, so a walker that has
//                moved by 1e-5 of its position keeps all its digits, where x_t - S_w / T would keep eleven of sixteen.
//                Thread w d + k reads X[t n d + w d + k]: a wave reads 512 contiguous bytes per step.
//   pool mean    one wave per coordinate: nok, mean = (sum_w S_w) / (T nok), the mean of the 2 nok half means (both v where every
//                used walker is constant at the one value v).  Lane l adds walkers
//                l, l + 64, ... in that order, then the 64 lane sums go through the fixed butterfly (wave_row.h: wave_sum).
//   centred      one thread per (w, k), t ascending: c_w(0) by one fma per step, sum (x - mean)^2, the half variances.
//   mean series  one wave per t: m_t = (sum_w x_t,w) / nok, w ascending.
//   lag          the hot path.  Workgroup = (walker block, 8 coordinates, 512 lags); thread (kk, j) holds the 16 sums c_w(tau),
//                tau = tau0 + 16 j + r, in registers and walks t ascending: per block of 16 steps it reads 16 values a = x_c[t + s]
//                and 16 new values of its window b = x_c[t + tau0 + 16 j + .] from LDS and makes 256 fmas,
//                c[r] = fma(a[s], b[s + r], c[r]).  Past the end of the series the image holds 0.0, which leaves a sum as it is:
//                the zero padding of the FFT route.  After the last t-block rho_w = c / c_w(0) joins the block's sum; the
//                walkers of a block are taken w ascending.  One thread owns a (walker block, k, tau) from the first step to
//                the last: there is nothing to combine across threads, no atomics, and the bits do not depend on the grid.
//   acf          one thread per (k, tau): the walker blocks in block order, / nused.
//   pool var     one wave per coordinate: nused, var, W, B, rhat, as pool mean adds.
//   tau          one thread per coordinate: the window rule over rho(0 .. L), tau, ess.
#pragma once
#include <hip/hip_runtime.h>

#include "chain_args.h"
#include "wave_row.h"

using namespace mcalf;

namespace {

__device__ __forceinline__ bool chain_used(const ChainArgs& a, int64_t w) { return !a.status || a.status[w] == 0; }
__device__ __forceinline__ double chain_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

}  // namespace

namespace mcalf {

__global__ __launch_bounds__(256) void mcalf_chain_sums_kernel(const ChainArgs a) {
    const size_t nd = (size_t)a.n * a.d, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nd) return;
    const int64_t T = a.T, h = T / 2;
    const double* x = a.X + i;
    const double x0 = x[0];
    double s = 0.0, sd = 0.0, s1 = 0.0, s2 = 0.0;
    bool konst = true;                                    // x_t == x_0 for every t (a NaN is equal to nothing: not constant)
    for (int64_t t = 0; t < T; ++t) {
        const double v = x[(size_t)t * nd];
        konst = konst && v == x0;
        s += v;
        sd += v - x0;
        if (t < h) s1 += v;
        if (t >= T - h) s2 += v;
    }
    // A constant series has its means by definition, not by a rounded sum, and its centred values are 0: c_w(0) == 0 exactly.
    a.sum[i] = s;
    a.kf[i] = konst ? 1.0 : 0.0;
    a.mu[i] = konst ? x0 : sd / (double)T;               // (x_0 of a constant series: pool mean compares them)
    a.hm[i] = konst ? x0 : s1 / (double)h;
    a.hm[nd + i] = konst ? x0 : s2 / (double)h;
}

__global__ __launch_bounds__(64) void mcalf_chain_pool_mean_kernel(const ChainArgs a) {
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t nd = (size_t)a.n * a.d;
    double s = 0.0, sh = 0.0, cnt = 0.0, allk = 1.0, lo = __builtin_inf(), hi = -__builtin_inf();
    for (int64_t w = l; w < a.n; w += 64) {
        if (!chain_used(a, w)) continue;
        const size_t i = (size_t)w * a.d + k;
        s += a.sum[i];
        sh += a.hm[i] + a.hm[nd + i];
        cnt += 1.0;
        const double m = a.mu[i];
        allk = a.kf[i] != 0.0 ? allk : 0.0;
        lo = m < lo ? m : lo;
        hi = m > hi ? m : hi;
    }
    s = wave_sum(s);
    sh = wave_sum(sh);
    cnt = wave_sum(cnt);
    allk = wave_min(allk);
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (l != 0) return;
    // every used walker constant at ONE value v (a frozen coordinate): the means are v, so that var is 0 and W is 0 exactly
    const bool frozen = cnt > 0.0 && allk != 0.0 && lo == hi;
    double* p = a.pool + (size_t)k * kChainPool;
    p[kPoolMean] = frozen ? lo : s / ((double)a.T * cnt);
    p[kPoolHalfMean] = frozen ? lo : sh / (2.0 * cnt);
    p[kPoolNok] = cnt;
}

__global__ __launch_bounds__(256) void mcalf_chain_centred_kernel(const ChainArgs a) {
    const size_t nd = (size_t)a.n * a.d, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nd) return;
    const int k = (int)(i % (size_t)a.d);
    const int64_t T = a.T, h = T / 2;
    const double dl = a.kf[i] != 0.0 ? 0.0 : a.mu[i], mean = a.pool[(size_t)k * kChainPool + kPoolMean], m1 = a.hm[i], m2 = a.hm[nd + i];
    const double* x = a.X + i;
    const double x0 = x[0];
    double c0 = 0.0, sq = 0.0, v1 = 0.0, v2 = 0.0;
    for (int64_t t = 0; t < T; ++t) {
        const double v = x[(size_t)t * nd];
        const double xc = (v - x0) - dl, dm = v - mean;
        c0 = __builtin_fma(xc, xc, c0);
        sq += dm * dm;
        if (t < h) { const double e = v - m1; v1 += e * e; }
        if (t >= T - h) { const double e = v - m2; v2 += e * e; }
    }
    a.c0[i] = c0;
    a.sq[i] = sq;
    a.hv[i] = v1 / (double)(h - 1);
    a.hv[nd + i] = v2 / (double)(h - 1);
}

__global__ __launch_bounds__(64) void mcalf_chain_mean_series_kernel(const ChainArgs a) {
    const size_t t = blockIdx.x, nd = (size_t)a.n * a.d;
    const double* row = a.X + t * nd;
    for (int k = threadIdx.x; k < a.d; k += 64) {
        double s = 0.0, cnt = 0.0;
        for (int64_t w = 0; w < a.n; ++w) {
            if (!chain_used(a, w)) continue;
            s += row[(size_t)w * a.d + k];
            cnt += 1.0;
        }
        a.mser[t * a.d + k] = s / cnt;
    }
}

__global__ __launch_bounds__(kChainBlock) void mcalf_chain_lag_kernel(const ChainArgs a) {
    __shared__ double xa[kChainKT * kChainTB];
    __shared__ double xb[kChainKT * kChainBRow];
    const int tid = threadIdx.x, kk = tid / kChainJ, j = tid % kChainJ;
    const int64_t w0 = (int64_t)blockIdx.x * kChainWalkerBlock, w1 = w0 + kChainWalkerBlock < a.n ? w0 + kChainWalkerBlock : a.n;
    const int64_t tau0 = (int64_t)blockIdx.y * kChainLT, T = a.T;
    const int k0 = (int)blockIdx.z * kChainKT, k = k0 + kk;
    const size_t nd = (size_t)a.n * a.d;
    const bool mine = k < a.d && tau0 + (int64_t)kChainR * j <= a.L;      // this thread has a lag to report
    // staging: element e of a t-block is (i, c) = (e / kChainKT, e % kChainKT): the 8 coordinates of a row are adjacent lanes
    const int sc = tid % kChainKT, si = tid / kChainKT;
    const bool skv = k0 + sc < a.d;
    double rs[kChainR];
#pragma unroll
    for (int r = 0; r < kChainR; ++r) rs[r] = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        if (!chain_used(a, w)) continue;                                  // (uniform over the workgroup)
        const size_t wk = (size_t)w * a.d + k0;
        const double smu = skv && a.kf[wk + sc] == 0.0 ? a.mu[wk + sc] : 0.0;   // delta_w; a constant series is all 0
        const double* xw = a.X + wk + sc;
        const double sx0 = skv ? xw[0] : 0.0;
        double c[kChainR];
#pragma unroll
        for (int r = 0; r < kChainR; ++r) c[r] = 0.0;
        for (int64_t t0 = 0; t0 < T - tau0; t0 += kChainTB) {
            for (int i = si; i < kChainTB; i += kChainBlock / kChainKT) {
                const int64_t t = t0 + i;
                xa[sc * kChainTB + i] = skv && t < T ? (xw[(size_t)t * nd] - sx0) - smu : 0.0;
            }
            for (int i = si; i < kChainBLog; i += kChainBlock / kChainKT) {
                const int64_t t = t0 + tau0 + i;
                xb[sc * kChainBRow + i + i / kChainR] = skv && t < T ? (xw[(size_t)t * nd] - sx0) - smu : 0.0;
            }
            __syncthreads();
            if (mine) {
                // register blocks that still meet a product inside the series: t + tau0 <= T - 1
                const int64_t left = T - tau0 - t0;
                const int nq = (int)((left < kChainTB ? left : kChainTB) + kChainR - 1) / kChainR;
                const double* bp = xb + kk * kChainBRow + (kChainR + 1) * j;
                const double* ap = xa + kk * kChainTB;
                double b[2 * kChainR];
#pragma unroll
                for (int u = 0; u < kChainR; ++u) b[u] = bp[u];
#pragma unroll 2
                for (int q = 0; q < nq; ++q) {
#pragma unroll
                    for (int u = 0; u < kChainR; ++u) b[kChainR + u] = bp[(kChainR + 1) * (q + 1) + u];
#pragma unroll
                    for (int s = 0; s < kChainR; ++s) {
                        const double av = ap[kChainR * q + s];
#pragma unroll
                        for (int r = 0; r < kChainR; ++r) c[r] = __builtin_fma(av, b[s + r], c[r]);
                    }
#pragma unroll
                    for (int u = 0; u < kChainR; ++u) b[u] = b[kChainR + u];
                }
            }
            __syncthreads();
        }
        if (mine) {
            const double c0 = a.c0[wk + kk];
            if (c0 != 0.0) {                                              // (a NaN is not 0: it stays in and makes the coordinate NaN)
#pragma unroll
                for (int r = 0; r < kChainR; ++r) rs[r] += c[r] / c0;
            }
        }
    }
    if (!mine) return;
    double* out = a.part + ((size_t)blockIdx.x * a.d + k) * (size_t)(a.L + 1);
#pragma unroll
    for (int r = 0; r < kChainR; ++r) {
        const int64_t tau = tau0 + (int64_t)kChainR * j + r;
        if (tau <= a.L) out[tau] = rs[r];
    }
}

__global__ __launch_bounds__(256) void mcalf_chain_acf_kernel(const ChainArgs a) {
    const size_t L1 = (size_t)(a.L + 1), i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.d * L1) return;
    const size_t k = i / L1;
    double s = 0.0;
    for (int b = 0; b < a.nblocks; ++b) s += a.part[(size_t)b * a.d * L1 + i];
    const double r = s / a.pool[k * kChainPool + kPoolNused];
    a.rho[i] = r;
    if (a.acf) a.acf[i] = r;
}

__global__ __launch_bounds__(64) void mcalf_chain_pool_var_kernel(const ChainArgs a) {
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t nd = (size_t)a.n * a.d;
    double* p = a.pool + (size_t)k * kChainPool;
    const double hbar = p[kPoolHalfMean];
    double sq = 0.0, sw = 0.0, sb = 0.0, used = 0.0;
    for (int64_t w = l; w < a.n; w += 64) {
        if (!chain_used(a, w)) continue;
        const size_t i = (size_t)w * a.d + k;
        sq += a.sq[i];
        sw += a.hv[i] + a.hv[nd + i];
        const double e1 = a.hm[i] - hbar, e2 = a.hm[nd + i] - hbar;
        sb += e1 * e1 + e2 * e2;
        if (a.c0[i] != 0.0) used += 1.0;
    }
    sq = wave_sum(sq);
    sw = wave_sum(sw);
    sb = wave_sum(sb);
    used = wave_sum(used);
    if (l != 0) return;
    p[kPoolNused] = used;
    if (a.mean_series) return;
    const double nok = p[kPoolNok], h = (double)(a.T / 2);
    const double W = sw / (2.0 * nok), B = h * (sb / (2.0 * nok - 1.0));
    double* st = a.stats + (size_t)k * 6;
    st[0] = p[kPoolMean];
    st[1] = nok > 0.0 ? sq / ((double)a.T * nok - 1.0) : chain_nan();
    st[4] = W == 0.0 ? chain_nan() : sqrt(((h - 1.0) / h * W + B / h) / W);
}

__global__ __launch_bounds__(64) void mcalf_chain_tau_kernel(const ChainArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.d) return;
    const double* rho = a.rho + (size_t)k * (size_t)(a.L + 1);
    double s = 0.0, tau = 0.0;
    int64_t M = a.L;
    int reached = 0;
    for (int64_t m = 0; m <= a.L; ++m) {
        s += rho[m];
        tau = 2.0 * s - 1.0;
        if ((double)m >= a.c * tau) { M = m; reached = 1; break; }
    }
    double* st = a.stats + (size_t)k * 6;
    int32_t* in = a.info + (size_t)k * 4;
    const double* p = a.pool + (size_t)k * kChainPool;
    if (a.mean_series) {
        st[3] = tau;
        in[1] = (int32_t)M;
        in[3] |= reached << 1;
    } else {
        st[2] = tau;
        st[5] = p[kPoolNok] * (double)a.T / tau;
        in[0] = (int32_t)M;
        in[2] = (int32_t)p[kPoolNused];
        in[3] = reached;
    }
}

__global__ __launch_bounds__(256) void mcalf_chain_add_int_kernel(const ChainAddArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)a.n) a.dst[i] += a.src[i];
}

const void* chain_kernel_ptr(ChainKernel k) {
    static const void* const table[] = {(const void*)&mcalf_chain_sums_kernel, (const void*)&mcalf_chain_pool_mean_kernel,
                                        (const void*)&mcalf_chain_centred_kernel, (const void*)&mcalf_chain_mean_series_kernel,
                                        (const void*)&mcalf_chain_lag_kernel, (const void*)&mcalf_chain_acf_kernel,
                                        (const void*)&mcalf_chain_pool_var_kernel, (const void*)&mcalf_chain_tau_kernel,
                                        (const void*)&mcalf_chain_add_int_kernel};   // in the order of enum ChainKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kChainKernelCount, "one entry per ChainKernel");
    return table[k];
}
}  // namespace mcalf
