// lnprior of ONE row by ONE wave64, for the kernels that already hold the row (prior_kernels.hip, ns_kernels.hip,
// ens_kernels.hip), in the style of wave_row.h: lane k owns coordinates k, k + 64, ...; the result is wave-uniform.
//   lnprior = -inf                                                    if an entry is NaN or outside its box
//           = sum over sigma[k] > 0 of -0.5 (((theta_k - mu_k) / sigma_k)^2 + c_k)   otherwise   (hires_fitter.py:230)
// The sequence (include/mcalf_hip.h; tests/prior_reference.py restates it in numpy), every step ONE rounded IEEE operation:
//   theta_k = row_k, or with from_cube  u_k (hi_k - lo_k) + lo_k  -- multiply and add rounded separately, the arithmetic of
//             sample_param() / mcalf_scale_cube_kernel
//   d = (theta_k - mu_k) / sigma_k;  dd = d d;  s = dd + c_k;  term = -0.5 s
//   a lane adds its terms in index order onto +0.0 (coordinates with sigma[k] == 0 are skipped, not added as zeros); the 64 lane
//   sums go through wave_sum.
// The function carries its own contraction switch: fit_kernels.hip-style files leave contraction to FMA on.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <hip/hip_runtime.h>

#include "prior_args.h"
#include "wave_row.h"

namespace mcalf {

__device__ __forceinline__ double row_lnprior(const PriorDev& p, const double* row, int from_cube) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kPriorWave - 1);
    int bad = 0;
    double acc = 0.0;
    for (int k = lane; k < p.ndim; k += kPriorWave) {
        const double v = row[k], lo = p.lo[k], hi = p.hi[k];
        double th = v;
        if (from_cube) {
            bad |= outside_unit(v);
            const double scaled = v * (hi - lo);
            th = scaled + lo;
        } else {
            bad |= (v >= lo && v <= hi) ? 0 : 1;
        }
        if (p.mu) {
            const double sg = p.sigma[k];
            if (sg > 0.0) {
                const double d = (th - p.mu[k]) / sg;
                const double dd = d * d;
                const double s = dd + p.c[k];
                const double term = -0.5 * s;
                acc = acc + term;
            }
        }
    }
    const double total = uniform(wave_sum(acc));
    return __any(bad) ? -__builtin_inf() : total;
}

}  // namespace mcalf
