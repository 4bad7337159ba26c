// What the posterior-band kernels (band_kernels.hip) and their host side (host_band.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_band.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"

namespace mcalf {

constexpr int kBandStrip = 64;                    // pixels per strip: one lane owns one pixel, a wave reads 512 contiguous bytes of a row
constexpr int kBandRowBlock = 256;                // rows per block of the two moment passes: THE unit of the fixed reduction order
constexpr int kBandMomentThreads = 256;           // four waves, wave w sums rows [64 w, 64 w + 64) of its block in row order
constexpr int kBandMomentWaves = kBandMomentThreads / 64;
static_assert(kBandRowBlock == kBandMomentWaves * 64, "one row block is 64 rows per wave");
constexpr int kBandMaxQ = 16;                     // quantiles per call
constexpr int kBandDigitBits = 4;                 // radix-select digit: 16 passes over the 64-bit key
constexpr int kBandDigits = 1 << kBandDigitBits;
constexpr int kBandSelectThreads = 1024;          // sixteen waves over the rows of one strip; wave w takes rows w, w + 16, ...
constexpr int kBandSelectWaves = kBandSelectThreads / 64;
constexpr int kBandSelectLoads = 16;              // rows a wave of the select kernel has in flight per pass iteration
// LDS of the select kernel: the digit counters of one quantile's two ranks, [rank][digit][lane] -- 2 x 16 x 64 x 4 B = 8 KiB
constexpr int64_t kBandMaxBytes = 4LL << 30;      // largest [batch][npix] matrix of doubles a call may ask for

// One call.  The partial sums and counts are [nblocks][npix], block b = rows [b kBandRowBlock, (b + 1) kBandRowBlock).
struct BandArgs {
    const double* M;          // model rows, row-major [batch, npix]
    double* part;             // [nblocks, npix] per-block sums (of x, then of (x - mean)^2), NaN entries left out
    long long* pcnt;          // [nblocks, npix] per-block counts of non-NaN entries
    double* mean;             // [npix]   (the caller's, or the context's when the caller wants none)
    double* var;              // [npix] or nullptr
    long long* nvalid;        // [npix]   (likewise)
    double* sel;              // [2 nq, npix] selected order statistics: row 2 j the lower rank of q[j], row 2 j + 1 the upper
    double* Q;                // [nq, npix] or nullptr
    long long batch;
    int npix, nstrips, nblocks, nq;
    double q[kBandMaxQ];      // by value: nothing of the caller's is read after the entry returns
};

// The kernels of band_kernels.hip; all take (const BandArgs a).
enum BandKernel {
    kBandSum,         // grid = nblocks * nstrips (strip fastest), kBandMomentThreads: per-block count and sum
    kBandMean,        // grid = ceil(npix / 256), 256 threads: blocks combined in block order -> nvalid, mean
    kBandSquares,     // as kBandSum: per-block sum of (x - mean)^2
    kBandVar,         // as kBandMean -> var
    kBandSelect,      // grid = nstrips * nq (strip fastest), kBandSelectThreads: MSB-first radix select of the two ranks of q[j]
    kBandInterp,      // grid = ceil(nq * npix / 256), 256 threads: lo + (hi - lo) * t
    kBandKernelCount
};
MCALF_INTERNAL const void* band_kernel_ptr(BandKernel k);

}  // namespace mcalf
