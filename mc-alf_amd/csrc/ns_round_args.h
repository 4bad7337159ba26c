// What the book-keeping kernels of a device-resident nested-sampling run (ns_round_kernels.hip) and their host side
// (host_nsrun.cpp) share: the argument block, the round record and the kernel handles.  Plain C++ -- host_nsrun.cpp is compiled
// without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"

namespace mcalf {

constexpr int kNsrWave = 64;                 // the row kernels: ONE wave per row, lane k owns coordinates k, k + 64, ...
constexpr int kNsrBlock = 256;               // threads of the rank, select, covariance, Cholesky and retire workgroups
constexpr int kNsrRankRows = 32;              // rows a rank workgroup ranks ...
constexpr int kNsrRankSlices = 8;             // ... each over this many slices of a staged tile of keys (rows x slices = kNsrBlock)
constexpr int kNsrChunks = 128;              // the survivors are summed in this many contiguous chunks (moments: a workgroup each)
constexpr int kNsrCovTile = 16;              // survivor rows a covariance workgroup stages in LDS at a time
constexpr int kNsrCovMaxDim = 256;           // widest row the covariance tile holds (kNsrCovTile x kNsrCovMaxDim doubles of LDS)
constexpr int64_t kNsrMaxLive = 262144;      // nlive cap: the rank is counted, nlive^2 comparisons a round
constexpr size_t kNsrCholLds = 61440;        // a packed triangle up to this many bytes (ndim <= 123) is factored in LDS, a larger one in HBM

// The round record: K + kNsrRecWords 8-byte words, copied to the host once per round.  Words [0, K): the keys of the dying rows
// in death order (doubles).  Then, from word K on:
enum NsrRec {
    kRecMaxKey,       // double: the largest live key AFTER the round (before it, when nothing was retired)
    kRecLmin,         // double: the round's threshold
    kRecNstarts,      // int64: rows strictly above the threshold (0: a plateau, nothing was retired)
    kRecBad,          // int64: replacements with status < 0 or not (L > lmin) (nonzero: nothing was retired)
    kRecFirstBad,     // int64: the first such row
    kRecNevals,       // int64: sum of the replacements' nevals
    kRecUnfinished,   // int64: replacements with status 0
    kRecR0,           // int64: rows with key <= lmin
    kNsrRecWords
};

struct NsrArgs {
    double *UL, *LL;                  // the live set [nlive][ndim], [nlive]
    double *UD, *LD;                  // the dead rows [max_dead][ndim], [max_dead]
    int32_t *rank, *order;            // [nlive] each: order[rank[i]] = i
    int32_t *dying, *pick;            // [K] each: what the round selected
    double* meanpart;                 // [kNsrChunks][ndim] per-chunk sums of the survivors' rows
    double* covpart;                  // [kNsrChunks][ndim (ndim + 1) / 2] per-chunk sums of centred products, packed lower triangle
    double* tri;                      // [ndim (ndim + 1) / 2] the triangle the Cholesky workgroup factors when it does not fit LDS
    double* var;                      // [ndim] the covariance's diagonal (the fallback's variances)
    double* D;                        // [ndim][ndim] the round's direction rows
    double *U0, *Lmin;                // the starts [K][ndim] and thresholds [K] run_ns reads
    uint64_t* sid;                    // [K] their stream ids
    const double *Un, *Ln;            // the replacements run_ns left [K][ndim], [K]
    const int32_t *status, *nevals;   // [K] each
    uint64_t* rec;                    // the round record (doubles and int64 by word)
    uint64_t seed, round;             // the Philox key word 0; rounds completed before this one
    int64_t ndead;                    // dead rows before this round
    int nlive, ndim, K;
    int chol_in_lds;                  // 1: the packed triangle fits kNsrCholLds and is factored in (dynamic) LDS
};

// The kernels of ns_round_kernels.hip; all take (const NsrArgs a).
enum NsrKernel {
    kNsrInit,         // grid = ceil(nlive / kNsrBlock), kNsrBlock threads: an initial row outside the cube takes logL = -inf
    kNsrRank,         // grid = ceil(nlive / kNsrRankRows), kNsrBlock threads: rank by counting over LDS-staged tiles of keys
    kNsrSelect,       // ONE workgroup of kNsrBlock threads: dying, lmin, r0, nstarts, picks, the record's first half
    kNsrMean,         // grid = kNsrChunks, kNsrWave threads: per-chunk sums of the survivors' rows
    kNsrCov,          // grid = kNsrChunks, kNsrBlock threads: per-chunk sums of centred products
    kNsrChol,         // ONE workgroup of kNsrBlock threads: covariance, jitter, Cholesky or the fallback; D
    kNsrGather,       // grid = K, kNsrWave threads: U0, Lmin, sid of the chains
    kNsrRetire,       // grid = min(K, 256) workgroups of kNsrBlock threads: the bad count, then dead rows out and replacements in
    kNsrFinal,        // grid = nlive, kNsrWave threads: the remaining live rows to the dead slots in key order
    kNsrKernelCount
};
MCALF_INTERNAL const void* nsr_kernel_ptr(NsrKernel k);

}  // namespace mcalf
