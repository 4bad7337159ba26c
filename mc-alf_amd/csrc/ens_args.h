// What the ensemble-sampler kernels (ens_kernels.hip) and their host side (host_ens.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_ens.cpp is compiled
// without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"
#include "prior_args.h"

namespace mcalf {

constexpr int kEnsWave = 64;             // threads per workgroup: ONE wave per walker, lane k owns coordinates k, k + 64, ...
constexpr int kEnsAux = 3;               // per-moving-walker scalars in `aux`: [0][m] the Hastings term, [1][m] ln zeta, [2][m] lnprior of
                                         // an inside trial (written and read under a Gaussian prior only)
constexpr uint64_t kEnsKey1 = 1;         // key word 1 of the ensemble's Philox streams (nested sampling's is 0)
constexpr uint64_t kEnsKey2 = 2;         // key word 1 of the swap rounds' streams (mcalf_tempered_batch)
constexpr int kEnsMaxTemps = 64;         // temperatures of one call at most: their beta travel in the argument block

// Status of a walker; the moves (MCALF_ENS_STRETCH / MCALF_ENS_DE of the public header).
enum { kEnsOk = 0, kEnsBadStart = -1 };
enum { kEnsStretch = 0, kEnsDE = 1 };

// (ens_ln(x), the fixed-sequence logarithm, and its constants: ens_ln.h, which hmc_kernels.hip includes as well)

// One half-step, or one swap round, of one call: T = ntemps temperatures of n walkers each (mcalf_ensemble_batch: T = 1 with
// beta[0] = 1).  Row t n + w is walker w of temperature t; a half-step moves the T m rows t n + half m + b, trial row t m + b
// (the logL launch between the propose and the decide kernel cuts its own blocks).
struct EnsArgs {
    const double* U0;         // the caller's starts [T n, ndim] (read by the start kernel only)
    double* U;                // the walkers, the caller's U rows [T n, ndim]
    double* L;                // their logL (untempered), the caller's logL rows [T n]
    int32_t *status, *naccept;   // the caller's rows [T n]
    int32_t* nswap;           // the caller's rows [(T - 1) n]: accepted swaps of position (t, w) with temperature t + 1; NULL at T = 1
    double* Y;                // the trial rows of the moving halves [T m, ndim], what the logL launch evaluates
    const double* LY;         // logL of the trial rows [T m], what it leaves
    double* aux;              // [kEnsAux][T m]
    int32_t* inside;          // [T m] 1: the trial row is a proposal inside the cube; 0: it is the walker's own point (rejected)
    double* CU;               // the chain slot this half-step fills after its decisions [chain_temps n, ndim]; NULL: none (or not wanted)
    double* CL;               // [T n], as CU
    uint64_t seed, step;      // the Philox key word 0; the global half-step s = 2 (first_iter + i) + h (the words: counter s + 1)
    uint64_t round;           // the swap round r (the swap kernel's words: counter r + 1)
    double scale;             // a of the stretch move, g of the DE move
    int n, m, ndim, move, half;
    int keep;                 // 1: this half-step ends an iteration whose state goes into the chain (CU / CL where given)
    int ntemps, chain_temps;  // T; the temperatures whose rows go into CU (the first ones)
    int pair0;                // the swap round's first pair (r mod 2): its pairs are (pair0 + 2 p, pair0 + 2 p + 1)
    double beta[kEnsMaxTemps];   // the inverse temperatures, [0, T) used
    PriorDev prior;           // prior.mu != NULL (a Gaussian prior is set): the accept rule gains lnprior(y) - lnprior(x), untempered
    double* PR;               // lnprior of the walkers [T n] (a workspace of the call; NULL without a Gaussian prior)
};

// The kernels of ens_kernels.hip; all take (const EnsArgs a), kEnsWave threads.
enum EnsKernel {
    kEnsStart,        // grid T n: U = U0, naccept 0 (nswap 0), status -1 for a start outside the cube or with a NaN, else 0; PR
    kEnsPropose,      // grid T m: the trial row of moving walker t n + half m + b, its Hastings term, ln zeta and inside flag
    kEnsDecide,       // grid T m: accept or reject it; with `keep`, the block then copies walkers b and m + b of its temperature into the chain slot
    kEnsSwap,         // grid (pairs of the round) n: one exchange between position (t, w) and its partner in temperature t + 1
    kEnsKernelCount
};
MCALF_INTERNAL const void* ens_kernel_ptr(EnsKernel k);

}  // namespace mcalf
