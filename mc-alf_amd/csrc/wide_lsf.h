// The kernels behind the fused one when the LSF is wider than a workgroup tile (included by kernels.hip, launched by host_wide.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"
#include "voigt_device.h"
#include "wave_util.h"
#include "sample_setup.h"

namespace mcalf {

// ---- LSF wider than a workgroup tile: two more kernels behind the fused one ---------------------------------------------
// The fused kernel convolves inside a 4096-pixel LDS tile, halo included.  A context whose LSF half-width does not fit
// one (a very finely sampled spectrum, a very coarse resolution: the reference simply builds a longer kernel,
// hires_fitter.py:458-464) runs the SAME fused kernel without its convolution and continuum -- the host passes it
// velstep = 1e300 (hires_fitter.py:445: no convolution while R <= velstep; JAX semantics: a kernel grid of half-width 0,
// i.e. the single tap 1), a fixed continuum of 1 -- into a buffer of
// unconvolved spectra [rows][npix], and these two kernels do the rest: the taps of every live point (any half-width up
// to the one provisioned from specres_max), then the periodic convolution, the continuum and the likelihood terms.
// The convolution is the fused kernel's scheme at a larger scale: a workgroup owns kWideBlockPix consecutive outputs,
// eight per thread, and walks over the taps in passes of kWideTapChunk -- per pass the flux window (outputs + taps of the
// pass, wrapped round the spectrum as often as it takes) and the taps are staged in LDS, the window in the mod-8 planar
// layout, and every thread slides an 8-register window over it: one LDS flux read and one broadcast weight per 8 FMAs.
// Every output accumulates its taps in tap order (tap 0 first), which is astropy's loop order and the order `bot` is
// formed in -- an absorber-free model therefore comes out as exactly 1.0, as it does from the fused kernel.
constexpr int kWideBlock = kWideBlockThreads;
constexpr int kWidePlane = (kWideBlockPix + kWideTapChunk + 16) / 8 + 2;      // 324: plane stride of the staged window
static_assert(kWideBlockPix == 8 * kWideBlock && kWideTapChunk % 8 == 0 && kWidePlane % 32 == 4, "wide convolution geometry");
__device__ __forceinline__ int wide_pos(int i) { return (i & 7) * kWidePlane + (i >> 3); }
__device__ __forceinline__ double wide_block_sum(double v, double* red, int tid) {      // fixed order (deterministic)
    v = wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWideBlock / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// Decode (R, continuum) of live point s as setup_sample() does (hires_fitter.py:412-425; mode OneComp: the row is (R, cont, N, z, b)).
__device__ __forceinline__ void wide_decode(const KArgs& a, long s, double& R, double& cont) {
    const int rowlen = (a.mode == kModeOneComp) ? 5 : a.ndim;
    const double* p = a.P + (size_t)s * rowlen;
    if (a.mode == kModeOneComp) { R = p[0]; cont = p[1]; return; }
    R = a.freespecres ? sample_param(a, p, 0) : a.specres_fixed;
    cont = a.freecont ? sample_param(a, p, a.freespecres ? 1 : 0) : a.contval_fixed;
}

// One workgroup per live point: its normalised Gaussian taps w[0 .. 2n] (astropy's Gaussian1DKernel divided by its sum),
// the sum `bot` astropy's loop divides by -- added up tap after tap, tap 0 first, the order the convolution's numerator
// chain runs in (as setup_sample() does for the fused kernel) -- and the header (continuum, bot, n, bad).
// kZeroPad (JAX semantics, hires_fitter.py:549-560,667-670): the kernel grid is FIXED at the context's half-width (from
// the largest resolution), the taps are exp(-k^2 / 2 sigma^2) divided by their sum and nothing else divides (bot = 1).
template <bool kZeroPad>
__global__ __launch_bounds__(kWideBlock) void mcalf_wide_taps_kernel(const KArgs a, double* taps, long tap_stride, SampleHdr* hdr) {
    __shared__ double red[kWideBlock / 64];
    const long s = blockIdx.x;
    const int tid = threadIdx.x;
    double R, cont;
    wide_decode(a, s, R, cont);
    const double sigma = (R / kFwhmToSigma) / a.velstep;         // :454
    long n = 0;
    bool bad = false;
    if (kZeroPad) {
        n = a.jax_half;                                          // :549-560 fixed grid
    } else if (R > a.velstep) {                                  // :445
        const double nd = ceil(kKernelReach * sigma);            // :458
        if (!(nd <= (double)a.n_cap)) bad = true;                // (beyond the half-width provisioned from specres_max; NaN too)
        else n = (long)nd;
    }
    double* w = taps + (size_t)s * tap_stride;
    // (the expressions of setup_sample(), so that a kernel that fits a tile and one that does not form their taps alike)
    const double inv2s2 = kZeroPad ? 1.0 / (2.0 * sigma * sigma) : 0.5 / (sigma * sigma);
    const double amp = kZeroPad ? 1.0 : 1.0 / (sqrt(2.0 * M_PI) * sigma);
    double part = 0.0;
    for (long k = tid; k <= 2 * n; k += kWideBlock) {
        const double dk = (double)(k - n);
        const double g = (n == 0 && !kZeroPad) ? 1.0 : exp_neg((dk * dk) * inv2s2) * amp;
        w[k] = g;
        part += g;
    }
    const double gsum = wide_block_sum(part, red, tid);
    for (long k = tid; k <= 2 * n; k += kWideBlock) w[k] = w[k] / gsum;     // normalize_kernel=True
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double bot = 0.0;                                        // tap order: a dependent chain of 2n + 1 additions, once per live point
        if (kZeroPad) bot = 1.0;                                 // (:670 normalises the kernel; jnp.convolve divides by nothing)
        else for (long k = 0; k <= 2 * n; ++k) bot += w[k];
        SampleHdr h;
        h.cont = cont; h.bot = bot; h.ncl = 0; h.n = (int)n; h.bad = bad ? 1 : 0; h.ngeneral = 0;
        hdr[s] = h;
    }
}

// Workgroup (blockIdx.x, blockIdx.y) = pixels [2048 x, 2048 x + 2048) of live point y:  model = (sum_k w_k flux[(i + k - n) mod
// npix]) / bot x continuum (astropy boundary='wrap', taps in window order; hires_fitter.py:463-464, :447), then the model
// row and / or the likelihood terms (:292-303) summed over the block into partial[y][x][4], which mcalf_finalize_kernel adds up.
// kZeroPad (JAX semantics): jnp.convolve(model, kernel, 'same') -- zeros outside the spectrum instead of the periodic
// window (:674) -- and the first / last n pixels reset to the unconvolved model (:677-681); nothing divides the sum.
template <bool kZeroPad>
__global__ __launch_bounds__(kWideBlock) void mcalf_wide_conv_kernel(const KArgs a, const double* flux, const double* taps, long tap_stride,
                                                                         const SampleHdr* hdr, int nblocks) {
    __shared__ double red[kWideBlock / 64];
    __shared__ double sF[8 * kWidePlane];
    __shared__ double sW[kWideTapChunk];
    const long s = blockIdx.y;
    const int tid = threadIdx.x;
    const long i0 = (long)blockIdx.x * kWideBlockPix;            // first output pixel of the workgroup
    const SampleHdr h = hdr[s];
    const long n = h.n, npix = a.npix, ntaps = 2 * n + 1;
    const double* f = flux + (size_t)s * npix;
    const double* w = taps + (size_t)s * tap_stride;
    double top[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) top[m] = 0.0;
    if (!h.bad) {                                                // (workgroup-uniform)
        for (long k0 = 0; k0 < ntaps; k0 += kWideTapChunk) {
            const int kt = (int)min((long)kWideTapChunk, ntaps - k0);       // taps of this pass
            // window element e of the pass = flux[(i0 - n + k0 + e) mod npix]: output 8 t + m reads element 8 t + m + k at tap k0 + k
            if (kZeroPad) {
                const long first = i0 - n + k0;
                for (int e = tid; e < kWideBlockPix + kWideTapChunk + 16; e += kWideBlock) {
                    const long j = first + e;
                    sF[wide_pos(e)] = (e < kWideBlockPix + kt && j >= 0 && j < npix) ? f[j] : 0.0;      // :674 zero padding
                }
            } else {
                long src = (i0 - n + k0 + tid) % npix;
                if (src < 0) src += npix;
                const long step = kWideBlock % npix;
                for (int e = tid; e < kWideBlockPix + kWideTapChunk + 16; e += kWideBlock) {
                    sF[wide_pos(e)] = (e < kWideBlockPix + kt) ? f[src] : 0.0;   // (past the pass's window: never multiplied by a tap)
                    src += step;
                    if (src >= npix) src -= npix;
                }
            }
            for (int k = tid; k < kWideTapChunk; k += kWideBlock) sW[k] = (k < kt) ? w[k0 + k] : 0.0;
            __syncthreads();
            double win[8];
            const double* fp = sF + tid;                         // element 8 tid + 8 c + r  ->  fp[r * kWidePlane + c]
#pragma unroll
            for (int m = 0; m < 8; ++m) win[m] = fp[m * kWidePlane];
            const double* wp = sW;
            for (int q0 = 0; q0 + 8 <= kt; q0 += 8) {            // whole groups of eight taps
                ++fp;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const double wgt = wp[r];
#pragma unroll
                    for (int m = 0; m < 8; ++m) top[m] = fma(win[(m + r) & 7], wgt, top[m]);
                    win[r] = fp[r * kWidePlane];
                }
                wp += 8;
            }
            {                                                    // the pass's last 0..7 taps: no zero-weight padding taps
                const int rem = kt & 7;                          // (workgroup-uniform)
                ++fp;
#pragma unroll
                for (int r = 0; r < 7; ++r) {
                    if (r >= rem) break;
                    const double wgt = wp[r];
#pragma unroll
                    for (int m = 0; m < 8; ++m) top[m] = fma(win[(m + r) & 7], wgt, top[m]);
                    win[r] = fp[r * kWidePlane];
                }
            }
            __syncthreads();                                     // every wave is past its reads before the next pass overwrites
        }
    }
    const bool reduces = a.mode == kModeLogL || a.mode == kModeChi2;
    double acc = 0.0, nnz = 0.0, c4 = 0.0, c5 = 0.0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const long i = i0 + 8 * tid + m;
        if (i >= npix) break;
        double mval = NAN;
        if (!h.bad) {
            mval = kZeroPad ? top[m] : top[m] / h.bot;
            if (kZeroPad && (i < n || i >= npix - n)) mval = f[i];       // :677-681 edge reset to the unconvolved model
            mval *= h.cont;                                      // :447 / :683
        }
        if (a.model) a.model[(size_t)s * npix + i] = mval;
        if (reduces) {
            const double d = a.obj[i] - mval;
            double term = a.ispec2[i] * (d * d);
            if (a.mode == kModeLogL) term = (term - a.lgis[i]) + a.log2pi;      // :294
            if (!isnan(term)) acc += term;                                    // np.nansum
            if (a.mode == kModeChi2 && mval != 0.0) nnz += 1.0;               // :241
            if (a.asymm) {                                                     // :298-302
                const double resid = d / a.err[i];
                if (resid > 4.0) c4 += 1.0;
                if (resid > 5.0) c5 += 1.0;
            }
        }
    }
    if (!reduces) return;                                        // (workgroup-uniform)
    acc = wide_block_sum(acc, red, tid);
    nnz = wide_block_sum(nnz, red, tid);
    if (a.asymm) { c4 = wide_block_sum(c4, red, tid); c5 = wide_block_sum(c5, red, tid); }
    if (tid == 0) {
        if (h.bad) { acc = INFINITY; nnz = 1.0; }               // not computed: logL = -inf, chi2 = +inf (as in the fused kernel)
        double* pr = a.partial + ((size_t)s * nblocks + blockIdx.x) * 4;
        pr[0] = acc; pr[1] = nnz; pr[2] = c4; pr[3] = c5;
    }
}

}  // namespace mcalf
