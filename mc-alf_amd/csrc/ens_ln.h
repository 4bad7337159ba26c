// The fixed-sequence logarithm of the samplers' kernels (ens_kernels.hip: ln z and ln zeta of the accept rules; hmc_kernels.hip:
// ln zeta and the polar method's ln q): its constants and the device function, operation for operation what
// tests/ens_reference.py restates in numpy.
//   e, f   x = f 2^e with f in [1, 2), from the bits;  if f > kEnsSqrt2: f <- 0.5 f (exact), e <- e + 1
//   r      = (f - 1) / (f + 1)             (f - 1 is exact; |r| <= 0.1716)
//   s      = r r
//   p      = c9;  p <- p s + c_i for i = 8 .. 1, with c_i = 1 / (2 i + 1)  (each step a product and a sum)
//   t      = r + r;  lnf = t + (t s) p     (the odd series 2 r (1 + s / 3 + s^2 / 5 + ...), cut after s^9 / 19: the next
//                                           term is below 2.3e-17 of the sum)
//   ln x   = e kEnsLn2Hi + (lnf + e kEnsLn2Lo)    (kEnsLn2Hi has 21 trailing zero bits: e kEnsLn2Hi is exact)
// The function carries its own contraction switch, as row_lnprior of prior_device.h does; the files that include it have
// switched contraction to FMA off for the whole file anyway.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <hip/hip_runtime.h>

namespace mcalf {

constexpr double kEnsSqrt2 = 0x1.6a09e667f3bcdp+0;
constexpr double kEnsLn2Hi = 0x1.62e42feep-1, kEnsLn2Lo = 0x1.a39ef35793c76p-33;
constexpr int kEnsLnTerms = 9;

// ln x for normal positive x.
__device__ __forceinline__ double ens_ln(double x) {
#pragma clang fp contract(off)
    const long long b = __double_as_longlong(x);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    double f = __longlong_as_double((b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);
    if (f > kEnsSqrt2) { f = f * 0.5; e += 1; }
    const double r = (f - 1.0) / (f + 1.0);
    const double s = r * r;
    double p = 1.0 / (2 * kEnsLnTerms + 1);
#pragma unroll
    for (int i = kEnsLnTerms - 1; i >= 1; --i) p = p * s + 1.0 / (2 * i + 1);
    const double t = r + r;
    const double lnf = t + (t * s) * p;
    const double ed = (double)e;
    return ed * kEnsLn2Hi + (lnf + ed * kEnsLn2Lo);
}

}  // namespace mcalf
