// What the ensemble-sampler kernels (ens_kernels.hip) and their host side (host_ens.cpp) share: the argument block, the
// workspace layout, the constants of the fixed-sequence logarithm and the kernel handles.  Plain C++ -- host_ens.cpp is compiled
// without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"

namespace mcalf {

constexpr int kEnsWave = 64;             // threads per workgroup: ONE wave per walker, lane k owns coordinates k, k + 64, ...
constexpr int kEnsAux = 2;               // per-moving-walker scalars in `aux`: [0][m] the Hastings term, [1][m] ln zeta
constexpr uint64_t kEnsKey1 = 1;         // key word 1 of the ensemble's Philox streams (nested sampling's is 0)

// Status of a walker; the moves (MCALF_ENS_STRETCH / MCALF_ENS_DE of the public header).
enum { kEnsOk = 0, kEnsBadStart = -1 };
enum { kEnsStretch = 0, kEnsDE = 1 };

// ens_ln(x), x normal and positive: a fixed sequence of IEEE operations (tests/ens_reference.py restates it in numpy).
//   e, f   x = f 2^e with f in [1, 2), from the bits;  if f > kEnsSqrt2: f <- 0.5 f (exact), e <- e + 1
//   r      = (f - 1) / (f + 1)             (f - 1 is exact; |r| <= 0.1716)
//   s      = r r
//   p      = c9;  p <- p s + c_i for i = 8 .. 1, with c_i = 1 / (2 i + 1)  (each step a product and a sum)
//   t      = r + r;  lnf = t + (t s) p     (the odd series 2 r (1 + s / 3 + s^2 / 5 + ...), cut after s^9 / 19: the next
//                                           term is below 2.3e-17 of the sum)
//   ln x   = e kEnsLn2Hi + (lnf + e kEnsLn2Lo)    (kEnsLn2Hi has 21 trailing zero bits: e kEnsLn2Hi is exact)
constexpr double kEnsSqrt2 = 0x1.6a09e667f3bcdp+0;
constexpr double kEnsLn2Hi = 0x1.62e42feep-1, kEnsLn2Lo = 0x1.a39ef35793c76p-33;
constexpr int kEnsLnTerms = 9;

// One half-step of one call (all `m` moving walkers of it: the logL launch between the two kernels cuts its own blocks).
struct EnsArgs {
    const double* U0;         // the caller's starts [n, ndim] (read by the start kernel only)
    double* U;                // the walkers, the caller's U rows [n, ndim]
    double* L;                // their logL, the caller's logL rows [n]
    int32_t *status, *naccept;   // the caller's rows [n]
    double* Y;                // the trial rows of the moving half [m, ndim], what the logL launch evaluates
    const double* LY;         // logL of the trial rows [m], what it leaves
    double* aux;              // [kEnsAux][m]
    int32_t* inside;          // [m] 1: the trial row is a proposal inside the cube; 0: it is the walker's own point (rejected)
    double* CU;               // the chain slot this half-step fills after its decisions [n, ndim]; NULL: none (or not wanted)
    double* CL;               // [n], as CU
    uint64_t seed, step;      // the Philox key word 0; the global half-step s = 2 (first_iter + i) + h (the words: counter s + 1)
    double scale;             // a of the stretch move, g of the DE move
    int n, m, ndim, move, half;
    int keep;                 // 1: this half-step ends an iteration whose state goes into the chain (CU / CL where given)
};

// The kernels of ens_kernels.hip; all take (const EnsArgs a), kEnsWave threads.
enum EnsKernel {
    kEnsStart,        // grid n: U = U0, naccept 0, status -1 for a start outside the cube or with a NaN, else 0
    kEnsPropose,      // grid m: the trial row of moving walker half m + block, its Hastings term, ln zeta and inside flag
    kEnsDecide,       // grid m: accept or reject it; with `keep`, block b then copies walkers b and m + b into the chain slot
    kEnsKernelCount
};
MCALF_INTERNAL const void* ens_kernel_ptr(EnsKernel k);

}  // namespace mcalf
