// What the Hamiltonian Monte Carlo kernels (hmc_kernels.hip) and their host side (host_hmc.cpp) share: the argument blocks, the
// workspace layout and the kernel handles.  Plain C++ -- host_hmc.cpp is compiled without the HIP language mode.
// Not itself part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.  It does include
// kernel_args.h, which is hashed, for MCALF_INTERNAL alone -- as ens_args.h, ns_args.h and prior_args.h do -- and changes nothing there.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"
#include "prior_args.h"

namespace mcalf {

constexpr int kHmcWave = 64;             // threads per workgroup: ONE wave per walker, lane k owns coordinates k, k + 64, ...
constexpr uint64_t kHmcKey = 4;          // key word 1 of the sampler's Philox streams (0 .. 3: the slice step, the ensemble, its swaps, the run)
constexpr uint64_t kHmcDecision = 1ull << 63;   // counter word 1 of a walker's decision block (a momentum block: (attempt << 32) | k)
constexpr int kHmcAttempts = 16;         // Philox blocks one momentum may take: 32 candidate pairs of the polar method
constexpr int kHmcAux = 2;               // per-walker scalars in `aux`: [0][n] K0 of the trajectory, [1][n] lnprior of the walker
constexpr int kHmcPut = 448;             // 64-bit words one put kernel carries in its argument block: 3600 bytes with its header, under the
                                         // 4 KB a kernel's arguments may take

enum { kHmcOk = 0, kHmcBadStart = -1 };

// One kernel of one call over the n walkers: row w of every array is walker w.  The gradient launch between two kernels reads
// the theta rows TH and leaves logL in LY (the start's: in L itself) and the gradient row, in theta coordinates, in GY.
struct HmcArgs {
    const double* U0;         // the caller's starts [n, ndim] (read by the start kernel only)
    double* U;                // the walkers, the caller's U rows [n, ndim]
    double* L;                // their logL, the caller's logL rows [n]
    int32_t *status, *naccept, *ndead;   // the caller's rows [n]
    double* G;                // the walkers' cube gradient g [n, ndim], kept across iterations
    double* R;                // the momenta [n, ndim]
    double* Y;                // the trajectories' positions [n, ndim]; a dead trajectory's row is the walker's own point
    double* TH;               // theta(Y) [n, ndim]: what the gradient launch evaluates
    const double* LY;         // logL of the theta rows [n], what it leaves
    const double* GY;         // and their gradient rows [n, ndim]
    double* aux;              // [kHmcAux][n]
    int32_t* dead;            // [n] 1: the trajectory is dead (or the walker never moves)
    const double* scale;      // the per-coordinate lengths [ndim], on the device
    const uint64_t* wid;      // the walker ids [n], on the device; NULL: 0 .. n - 1
    double* CU;               // the chain slot the decide kernel fills [n, ndim]; NULL: none (or not wanted)
    double* CL;               // [n], as CU
    uint64_t seed, iter;      // the Philox key word 0; the global iteration g = first_iter + i (the words: counter g + 1)
    double eps, jitter;
    int n, ndim;
    int slot, prior_int;      // the ncomp slot (frozen); 1: the cube transform truncates it
    PriorDev prior;           // prior.mu != NULL (a Gaussian prior is set): its gradient joins g, its value the accept rule
};

// Host words into device memory through the argument block: the call's scale and walker ids never wait for a copy engine and
// the caller's arrays are free when the entry returns.  A call issues ceil(ndim / kHmcPut) such launches for scale (one, up to
// ndim 448) and, where wid is given, ceil(n / kHmcPut) for the ids (10 at 4096 walkers), once, ahead of the start; a call
// without wid issues none for the ids.
struct HmcPutArgs {
    uint64_t* dst;
    int count;                // words of v in use
    uint64_t v[kHmcPut];
};

// The kernels of hmc_kernels.hip; all but kHmcPutWords take (const HmcArgs a), grid n, kHmcWave threads.
enum HmcKernel {
    kHmcStart,        // behind the start's gradient launch: U = U0, g, lnprior, status, naccept 0, ndead 0
    kHmcDraw,         // the momenta, K0, the first half kick, the drift; Y, TH and the dead flag
    kHmcStep,         // behind a launch that is not a trajectory's last: the two half kicks around it and the next drift; Y, TH, dead
    kHmcDecide,       // behind the last launch: the last half kick, K1, accept or reject, ndead; the chain slot
    kHmcPutWords,     // (const HmcPutArgs p), one block of kHmcPut threads
    kHmcKernelCount
};
MCALF_INTERNAL const void* hmc_kernel_ptr(HmcKernel k);

}  // namespace mcalf
