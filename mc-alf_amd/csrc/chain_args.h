// What the chain-diagnostics kernels (chain_kernels.h) and their host side (host_chain.h) share: the argument block, the
// workspace layout, the tile constants and the kernel handles.  Plain C++ -- host_chain.h is compiled without the HIP
// language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"

namespace mcalf {

// The lag kernel's tile.  A workgroup of kChainBlock threads owns kChainWalkerBlock consecutive walkers, kChainKT coordinates
// and kChainLT lags; thread (kk, j) = (tid / kChainJ, tid % kChainJ) owns coordinate k0 + kk and the kChainR consecutive lags
// tau0 + kChainR j + r.  The centred series are staged kChainTB steps at a time.
constexpr int kChainBlock = 256;
constexpr int kChainKT = 8;                          // coordinates per workgroup: 64 contiguous bytes of a chain row
constexpr int kChainJ = kChainBlock / kChainKT;      // 32 lag sub-tiles: a half-wave is the 32 sub-tiles of ONE coordinate
constexpr int kChainR = 16;                          // lags per thread, and steps of t per register block
constexpr int kChainLT = kChainJ * kChainR;          // 512 lags per workgroup
constexpr int kChainTB = 192;                        // steps of t staged at a time (a multiple of kChainR)
constexpr int kChainWalkerBlock = 64;                // walkers whose rho_w a workgroup adds up, w ascending; the blocks are added in block order
// LDS image of a t-block.  A: x_c[t0 + i], i < kChainTB, row stride kChainTB.  B: x_c[t0 + tau0 + i], i < kChainTB + kChainLT,
// with one double of padding after every kChainR: logical i sits at i + i / kChainR, so the windows of the 32 sub-tiles of a
// coordinate start 17 doubles apart and a half-wave's ds_read_b64 touches 32 different bank pairs.
constexpr int kChainBLog = kChainTB + kChainLT;                  // 704
constexpr int kChainBRow = kChainBLog + kChainBLog / kChainR;    // 748
static_assert(kChainTB % kChainR == 0 && kChainLT % kChainR == 0, "whole register blocks");
static_assert((size_t)kChainKT * (kChainTB + kChainBRow) * sizeof(double) <= 64 * 1024, "the t-block fits static LDS");

constexpr int kChainPool = 8;     // doubles per coordinate in `pool`: see ChainArgs
enum { kPoolMean, kPoolHalfMean, kPoolNok, kPoolNused, kPoolCount_ };

// One statistics pass over a chain X [T][n][d] (row (t, w, .) is d contiguous doubles).  The per-walker arrays are [n][d].
struct ChainArgs {
    const double* X;
    const int32_t* status;    // [n] or NULL (all walkers used)
    double* sum;              // sum_t x_t
    double* kf;               // 1.0 where x_t == x_0 for every t (a constant series), else 0.0
    double* mu;               // delta_w = (sum (x_t - x_0)) / T, the centring of the ACF; x_0 for a constant series (and so the half means)
    double* c0;               // c_w(0) = sum_t (x_t - mu_w)^2, t ascending, one fma per step: the lag kernel's tau = 0 sum, bit for bit
    double* sq;               // sum_t (x_t - mean)^2, mean the pooled mean
    double* hm;               // [2][n][d] means of the first and the last h = T / 2 states
    double* hv;               // [2][n][d] their variances (ddof 1), two-pass
    double* pool;             // [d][kChainPool]: pooled mean, mean of the 2 nok half means, nok, nused (counts as doubles)
    double* mser;             // [T][d] the series of ensemble means over the used walkers
    double* part;             // [nblocks][d][L + 1]: per walker block the sum of rho_w(tau) over its used walkers, w ascending
    double* rho;              // [d][L + 1] the walker-averaged ACF
    double* stats;            // [d][6] mean, var, tau, tau_mean, rhat, ess
    int32_t* info;            // [d][4] M, M_mean, nused, flags
    double* acf;              // [d][L + 1] or NULL
    int64_t T, n, L;
    int d, nblocks;
    int mean_series;          // 1: this pass is over the ensemble-mean series (n = 1): its tau goes to tau_mean, M_mean, flag bit 1
    double c;
};

// The kernels of chain_kernels.h; all take (const ChainArgs a).
enum ChainKernel {
    kChainSums,       // grid ceil(n d / 256), 256 threads: per (w, k) sum, delta and the two half means, t ascending
    kChainPoolMean,   // grid d, 64 threads: nok, the pooled mean and the mean of the half means over the used walkers
    kChainCentred,    // grid ceil(n d / 256), 256 threads: per (w, k) c0, sq and the two half variances, t ascending
    kChainMeanSeries, // grid T, 64 threads: m_t per coordinate, w ascending
    kChainLag,        // grid (walker blocks, lag tiles, coordinate tiles), kChainBlock threads: the lag pass
    kChainAcf,        // grid ceil(d (L + 1) / 256), 256 threads: the blocks in block order, / nused
    kChainPoolVar,    // grid d, 64 threads: nused, var, W, B, rhat
    kChainTau,        // grid ceil(d / 64), 64 threads: the window rule, tau, ess
    kChainAddInt,     // (const ChainAddArgs): dst[i] += src[i]
    kChainKernelCount
};
struct ChainAddArgs { int32_t* dst; const int32_t* src; int64_t n; };
MCALF_INTERNAL const void* chain_kernel_ptr(ChainKernel k);

}  // namespace mcalf
