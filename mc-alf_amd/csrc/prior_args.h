// What the prior kernel (prior_kernels.hip), the samplers' kernels that evaluate the prior of a row they hold (ns_kernels.hip,
// ens_kernels.hip) and the host side (host_prior.cpp, host_ns.cpp, host_ens.cpp) share: the prior block, the argument block of
// mcalf_lnprior_kernel, the kernel handle, and the checks of mcalf_set_gauss_prior that need no device.  Plain C++ -- the host
// files are compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "kernel_args.h"

namespace mcalf {

constexpr int kPriorWave = 64;           // threads per workgroup: ONE wave per row, lane k owns coordinates k, k + 64, ...

// The prior of a context as the device sees it: the box of mcalf_set_prior and the Gaussian factors of mcalf_set_gauss_prior.
// mu == NULL: no Gaussian is set (sigma and c are NULL too) -- the samplers' kernels then take the code path they had before
// there was one, and lnprior is 0 / -inf by the box test alone.
struct PriorDev {
    const double *lo, *hi;    // the box [ndim] each
    const double *mu, *sigma, *c;   // [ndim] each; sigma[k] == 0: no Gaussian on k; c[k] = ln(2 pi sigma[k]^2), from the host
    int ndim;
};

// One call of mcalf_lnprior_kernel: grid = nrows, kPriorWave threads.
struct PriorArgs {
    PriorDev prior;
    const double* rows;       // [nrows, ndim]: parameter rows, or unit-cube rows with from_cube
    double* out;              // [nrows]
    int from_cube;
};
MCALF_INTERNAL const void* prior_kernel_ptr();

// What mcalf_set_gauss_prior refuses about its arrays, in the order it looks: 0, or -1 with the message (which names the argument
// and the index) in `msg`.  `slot` is the ncomp slot.  No device, no context: a stand-alone program can run it.
inline int gauss_prior_check(const double* mu, const double* sigma, int ndim, int slot, char* msg, size_t len) {
    for (int k = 0; k < ndim; ++k) {
        if (!std::isfinite(sigma[k]) || sigma[k] < 0.0) {
            snprintf(msg, len, "sigma[%d] must be finite and >= 0 (0: no Gaussian on this parameter), got %g", k, sigma[k]);
            return -1;
        }
        if (sigma[k] > 0.0 && !std::isfinite(mu[k])) {
            snprintf(msg, len, "mu[%d] must be finite where sigma[%d] > 0, got %g", k, k, mu[k]);
            return -1;
        }
        if (sigma[k] > 0.0 && k == slot) {
            snprintf(msg, len, "sigma[%d] > 0 puts a Gaussian on the ncomp slot (parameter %d), which the box truncates to an integer: "
                     "a density on it has no defined mass", k, k);
            return -1;
        }
    }
    return 0;
}

// c[k] = ln(2 pi sigma[k]^2) for sigma[k] > 0, else 0: computed ONCE, on the host, and stored -- the kernels and the numpy
// restatement (tests/prior_reference.py) take these bits.  Returns the number of Gaussian coordinates.
inline int gauss_prior_constants(const double* sigma, int ndim, double* c) {
    int n = 0;
    for (int k = 0; k < ndim; ++k) {
        c[k] = sigma[k] > 0.0 ? std::log(2.0 * 3.14159265358979323846 * (sigma[k] * sigma[k])) : 0.0;
        n += sigma[k] > 0.0 ? 1 : 0;
    }
    return n;
}

}  // namespace mcalf
