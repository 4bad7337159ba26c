// What the nested-sampling kernels (ns_kernels.hip) and their host side (host_ns.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_ns.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"

namespace mcalf {

constexpr int kNsWave = 64;              // threads per workgroup: ONE wave per row (chain), lane k owns coordinates k, k + 64, ...
constexpr int kNsBrk = 3;                // per-row bracket in `brk`: [0][rows] tl, [1][rows] tr, [2][rows] t of the trial

// Status of a row.  0 while it is live (and at the end: max_steps reached).
enum { kNsLive = 0, kNsDone = 1, kNsBadStart = -1 };

// Philox4x64-10 (Salmon et al. 2011), the constants numpy's Philox bit generator uses.
constexpr uint64_t kPhiloxM0 = 0xD2E7470EE14C6C93ull, kPhiloxM1 = 0xCA5A826395121157ull;
constexpr uint64_t kPhiloxW0 = 0x9E3779B97F4A7C15ull, kPhiloxW1 = 0xBB67AE8584CAA73Bull;

// One call of the replacement primitive (all `nrows` rows of it: the logL launch between two kernels cuts its own blocks).
struct NsArgs {
    const double* U0;         // the caller's starts [nrows, ndim] (read by the start kernels only)
    const double* Lmin;       // the caller's constraints [nrows]
    const double* D;          // direction rows [ndirs, ndim]
    const uint64_t* sid;      // stream ids [nrows]
    double* U;                // the current point, the caller's U rows [nrows, ndim]
    double* L;                // its logL, the caller's logL rows [nrows]
    int32_t *status, *nevals, *moves;   // the caller's rows [nrows]
    double* Y;                // the trial rows [nrows, ndim], what the logL launch evaluates
    const double* LY;         // logL of the trial rows [nrows], what it leaves
    double* brk;              // per-row bracket [kNsBrk][nrows]
    int32_t* dir;             // [nrows] the row of D the chain moves along; -1: the next proposal draws one
    unsigned int* live;       // rows that proposed a trial in this step (integer counter)
    uint64_t seed;
    int nrows, ndim, ndirs, nmoves;
    int it;                   // the step, 1 .. max_steps (+ 1: the last trial is decided, nothing is proposed)
    int decide, propose;
};

// The kernels of ns_kernels.hip; all take (const NsArgs a), grid = nrows, kNsWave threads.
enum NsKernel {
    kNsStart,         // U = Y = U0, counters 0, no direction
    kNsStarted,       // after logL(Y): L = logL(U0); status -1 for a start outside the cube, with a NaN or not above Lmin
    kNsStep,          // decide on the trial of step it - 1, propose the trial of step it
    kNsKernelCount
};
MCALF_INTERNAL const void* ns_kernel_ptr(NsKernel k);

}  // namespace mcalf
