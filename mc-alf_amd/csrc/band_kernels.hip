// Per-pixel posterior bands of the model over the rows of a chain (host_band.cpp: mcalf_model_band_batch): count, mean,
// two-pass variance and exact quantiles of every column of the row-major matrix M[batch][npix] that the model launch leaves
// in device memory.  NaN entries are left out, per pixel (np.nanmean / np.nanvar / np.nanquantile).
//
// In every kernel ONE LANE OWNS ONE PIXEL: a wave reads 64 adjacent doubles of a row (512 contiguous bytes), and different
// waves / workgroups take fixed sets of rows of the same 64-pixel strip.  No floating-point atomics; every floating-point
// sum runs in one order that depends on neither the batch, the grid nor the outputs requested: rows are cut into blocks of
// kBandRowBlock, a block's four waves sum 64 consecutive rows each in row order and are added in wave order, the blocks
// are added in block order.  The radix histograms are integer counters in LDS (atomic adds of 1: exact).
#include <hip/hip_runtime.h>

#include "band_args.h"

using namespace mcalf;

namespace {

// Order-preserving 64-bit key of a double that is not NaN: negatives with every bit flipped, the others with the sign bit set.
__device__ __forceinline__ unsigned long long band_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double band_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// The rows of block `blk` this wave sums: [r0, r1).
__device__ __forceinline__ void band_wave_rows(const BandArgs& a, int blk, int wave, long long* r0, long long* r1) {
    const long long b0 = (long long)blk * kBandRowBlock + (long long)wave * 64;
    *r0 = b0 < a.batch ? b0 : a.batch;
    *r1 = b0 + 64 < a.batch ? b0 + 64 : a.batch;
}

// Per-block partial of one strip: kCentred = false, count and sum of x; true, sum of (x - mean)^2.
template <bool kCentred>
__device__ __forceinline__ void band_moment(const BandArgs& a) {
    __shared__ double sSum[kBandMomentWaves][kBandStrip];
    __shared__ int sCnt[kBandMomentWaves][kBandStrip];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = blockIdx.x % a.nstrips, blk = blockIdx.x / a.nstrips;
    const int pix = strip * kBandStrip + lane;
    const bool live = pix < a.npix;
    long long r0, r1;
    band_wave_rows(a, blk, wave, &r0, &r1);
    double mu = 0.0;
    if (kCentred && live) mu = a.mean[pix];
    double s = 0.0;
    int n = 0;
    if (live) {
        const double* col = a.M + (size_t)r0 * (size_t)a.npix + (size_t)pix;
        const int rows = (int)(r1 - r0);
        int r = 0;
        for (; r + 8 <= rows; r += 8) {                                            // eight independent loads in flight, added in row order
            double x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = col[(size_t)(r + j) * (size_t)a.npix];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = x[j] == x[j];
                const double d = kCentred ? x[j] - mu : x[j];
                s += ok ? (kCentred ? d * d : d) : 0.0;
                n += ok ? 1 : 0;
            }
        }
        for (; r < rows; ++r) {
            const double x = col[(size_t)r * (size_t)a.npix];
            const bool ok = x == x;
            const double d = kCentred ? x - mu : x;
            s += ok ? (kCentred ? d * d : d) : 0.0;
            n += ok ? 1 : 0;
        }
    }
    sSum[wave][lane] = s;
    sCnt[wave][lane] = n;
    __syncthreads();
    if (wave == 0 && live) {
        double t = sSum[0][lane];
        int c = sCnt[0][lane];
#pragma unroll
        for (int w = 1; w < kBandMomentWaves; ++w) { t += sSum[w][lane]; c += sCnt[w][lane]; }
        const size_t o = (size_t)blk * (size_t)a.npix + (size_t)pix;
        a.part[o] = t;
        if (!kCentred) a.pcnt[o] = c;
    }
}

// The blocks of one pixel, in block order.
template <bool kCentred>
__device__ __forceinline__ void band_combine(const BandArgs& a) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.npix) return;
    double s = 0.0;
    long long n = 0;
    for (int b = 0; b < a.nblocks; ++b) {
        const size_t o = (size_t)b * (size_t)a.npix + (size_t)pix;
        s += a.part[o];
        if (!kCentred) n += a.pcnt[o];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!kCentred) {
        a.nvalid[pix] = n;
        a.mean[pix] = n > 0 ? s / (double)n : nan;
    } else {
        n = a.nvalid[pix];
        a.var[pix] = n > 0 ? s / (double)n : nan;
    }
}

}  // namespace

__global__ __launch_bounds__(kBandMomentThreads) void mcalf_band_sum_kernel(const BandArgs a) { band_moment<false>(a); }
__global__ __launch_bounds__(kBandMomentThreads) void mcalf_band_squares_kernel(const BandArgs a) { band_moment<true>(a); }
__global__ __launch_bounds__(256) void mcalf_band_mean_kernel(const BandArgs a) { band_combine<false>(a); }
__global__ __launch_bounds__(256) void mcalf_band_var_kernel(const BandArgs a) { band_combine<true>(a); }

// Exact selection, one workgroup per (strip, quantile): the two order statistics numpy's linear rule reads for q[j] -- ranks
// floor(h) and min(floor(h) + 1, nvalid - 1) of the pixel's valid values, h = (nvalid - 1) q[j] -- by MSB-first radix select
// over the 64-bit key, kBandDigitBits at a time.  Every rank carries its own prefix (the key bits found so far) and its
// rank among the values that share it.  A pass: all sixteen waves count, for their rows, the next digit of the values that
// match a rank's prefix into sCnt[rank][digit][lane] (lane = pixel: the 64 lanes of a wave fall into distinct banks whatever
// their digits); then every wave walks its pixel's sixteen counters and extends prefix and rank -- each wave for itself, the
// state stays in registers.  After the last pass the prefix IS the key of the selected value.  NaNs are never counted.
__global__ __launch_bounds__(kBandSelectThreads) void mcalf_band_select_kernel(const BandArgs a) {
    __shared__ unsigned int sCnt[2][kBandDigits][kBandStrip];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = blockIdx.x % a.nstrips, j = blockIdx.x / a.nstrips;
    const int pix = strip * kBandStrip + lane;
    const bool live = pix < a.npix;
    const long long n = live ? a.nvalid[pix] : 0;
    long long k0 = 0, k1 = 0;                                                      // ranks still to go among the values under the prefix
    if (n > 0) {
        const double h = (double)(n - 1) * a.q[j];
        k0 = (long long)floor(h);
        k1 = k0 + 1 < n - 1 ? k0 + 1 : n - 1;
    }
    unsigned long long p0 = 0, p1 = 0;
    const double* col = a.M + (size_t)pix;
    unsigned int* flat = &sCnt[0][0][0];
    for (int shift = 64 - kBandDigitBits; shift >= 0; shift -= kBandDigitBits) {
        for (int i = threadIdx.x; i < 2 * kBandDigits * kBandStrip; i += kBandSelectThreads) flat[i] = 0u;
        __syncthreads();
        if (n > 0) {
            const bool first = shift == 64 - kBandDigitBits;
            const int up = first ? 0 : shift + kBandDigitBits;                     // (a shift by 64 is not defined: the first pass matches everything)
            for (long long r = wave; r < a.batch; r += (long long)kBandSelectLoads * kBandSelectWaves) {
                double x[kBandSelectLoads];                                        // (the pass is bound by load latency: many rows in flight)
#pragma unroll
                for (int u = 0; u < kBandSelectLoads; ++u) {
                    const long long rr = r + (long long)u * kBandSelectWaves;
                    x[u] = rr < a.batch ? col[(size_t)rr * (size_t)a.npix] : __longlong_as_double(0x7ff8000000000000ll);
                }
#pragma unroll
                for (int u = 0; u < kBandSelectLoads; ++u) {
                    if (x[u] == x[u]) {
                        const unsigned long long key = band_key(x[u]);
                        const int d = (int)((key >> shift) & (unsigned long long)(kBandDigits - 1));
                        if (first || ((key ^ p0) >> up) == 0) atomicAdd(&sCnt[0][d][lane], 1u);
                        if (first || ((key ^ p1) >> up) == 0) atomicAdd(&sCnt[1][d][lane], 1u);
                    }
                }
            }
        }
        __syncthreads();
        {
            long long c0 = 0, c1 = 0;
            int d0 = kBandDigits - 1, d1 = kBandDigits - 1;
            long long b0 = 0, b1 = 0;                                              // values under the prefix below the chosen digit
            bool f0 = false, f1 = false;
#pragma unroll
            for (int d = 0; d < kBandDigits; ++d) {
                const long long h0 = sCnt[0][d][lane], h1 = sCnt[1][d][lane];
                if (!f0 && c0 + h0 > k0) { f0 = true; d0 = d; b0 = c0; }
                if (!f1 && c1 + h1 > k1) { f1 = true; d1 = d; b1 = c1; }
                c0 += h0; c1 += h1;
            }
            p0 |= (unsigned long long)d0 << shift; k0 -= f0 ? b0 : 0;
            p1 |= (unsigned long long)d1 << shift; k1 -= f1 ? b1 : 0;
        }
        __syncthreads();                                                           // (the counters are zeroed again at the top)
    }
    if (wave == 0 && live) {
        a.sel[(size_t)(2 * j) * (size_t)a.npix + (size_t)pix] = band_unkey(p0);
        a.sel[(size_t)(2 * j + 1) * (size_t)a.npix + (size_t)pix] = band_unkey(p1);
    }
}

// numpy's "linear" rule on the two selected values: lo + (hi - lo) * t, t the fractional part of h = (nvalid - 1) q[j].
__global__ __launch_bounds__(256) void mcalf_band_interp_kernel(const BandArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.nq * a.npix) return;
    const int j = (int)(idx / a.npix);
    const long long pix = idx - (long long)j * a.npix;
    const long long n = a.nvalid[pix];
    double out = __longlong_as_double(0x7ff8000000000000ll);
    if (n > 0) {
        const double h = (double)(n - 1) * a.q[j];
        const double t = h - floor(h);
        const double lo = a.sel[(size_t)(2 * j) * (size_t)a.npix + (size_t)pix];
        const double hi = a.sel[(size_t)(2 * j + 1) * (size_t)a.npix + (size_t)pix];
        out = lo + (hi - lo) * t;
    }
    a.Q[(size_t)idx] = out;
}

namespace mcalf {
const void* band_kernel_ptr(BandKernel k) {
    static const void* const table[] = {(const void*)&mcalf_band_sum_kernel, (const void*)&mcalf_band_mean_kernel,
                                        (const void*)&mcalf_band_squares_kernel, (const void*)&mcalf_band_var_kernel,
                                        (const void*)&mcalf_band_select_kernel, (const void*)&mcalf_band_interp_kernel};   // in the order of enum BandKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kBandKernelCount, "one entry per BandKernel");
    return table[k];
}
}  // namespace mcalf
