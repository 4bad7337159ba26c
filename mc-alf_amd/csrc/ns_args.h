// What the nested-sampling kernels (ns_kernels.hip) and their host side (host_ns.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_ns.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"
#include "prior_args.h"

namespace mcalf {

constexpr int kNsWave = 64;              // threads per workgroup: ONE wave per row (chain), lane k owns coordinates k, k + 64, ...
constexpr int kNsBrk = 3;                // per-row bracket in `brk`: [0][rows] tl, [1][rows] tr, [2][rows] t of the trial
constexpr int kNsPackBlock = 1024;       // threads of the pack kernel's ONE workgroup: rows it scans per pass
constexpr int kNsPackInts = 3;           // per-row integers of the packing: [0][rows] stamp, [1][rows] slot, [2][rows] idx

// Status of a row.  0 while it is live (and at the end: max_steps reached).
enum { kNsLive = 0, kNsDone = 1, kNsBadStart = -1 };

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
    unsigned int* live;       // rows that proposed a trial in this step (integer counter; the pack kernel stores its count here)
    int32_t* stamp;           // [nrows] the step in which the row last proposed a trial; 0: not in this call
    int32_t* slot;            // [nrows] where the row's trial sits among the packed rows of the step it proposed in.  NULL: the
                              // trials are evaluated in place, LY is indexed by the row
    int32_t* idx;             // [nrows] the packed rows of the step: idx[s] is the row of slot s, ascending
    double* Yc;               // the packed trial rows [nrows, ndim], what the logL launch evaluates when the rows are packed
    uint64_t seed;
    PriorDev prior;           // prior.mu != NULL (a Gaussian prior is set): the constrained quantity is logL + lnprior
    int nrows, ndim, ndirs, nmoves;
    int it;                   // the step, 1 .. max_steps (+ 1: the last trial is decided, nothing is proposed)
    int decide, propose;
};

// The kernels of ns_kernels.hip; all take (const NsArgs a).  The row kernels: grid = nrows, kNsWave threads.
enum NsKernel {
    kNsStart,         // U = Y = U0, counters 0, no direction, no stamp
    kNsStarted,       // after logL(Y): L = logL(U0) (+ lnprior(U0) under a Gaussian prior); status -1 for a start outside the cube, with a NaN or not above Lmin
    kNsStep,          // decide on the trial of step it - 1 (its logL at LY[slot ? slot[row] : row]), propose the trial of step
                      // it and stamp the row with it
    kNsPack,          // ONE workgroup of kNsPackBlock threads: the rows stamped `it`, ascending, into idx / slot; their count
                      // into *live
    kNsGather,        // grid = the launch size n >= *live, kNsWave threads: Yc[s] = Y[idx[s]], and Y row 0 for s >= *live
    kNsKernelCount
};
MCALF_INTERNAL const void* ns_kernel_ptr(NsKernel k);

}  // namespace mcalf
