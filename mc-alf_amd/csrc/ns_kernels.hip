// Device side of the nested-sampling replacement primitive (mcalf_slice_replace_batch), for gfx950: a batch of chains in the
// unit cube, each moved by slice sampling along direction rows under a hard likelihood constraint L > Lmin.  The likelihood is
// the cube logL launch's (kernels.hip, issued by host_ns.cpp between two kernels of this file); what lives here is the per-row
// state machine that keeps the loop on the device: decide on the last trial, shrink the bracket or accept, propose the next.
//
//   ONE wave64 per row, lane k owns coordinates k, k + 64, ... (any ndim).  The chord of a line through the cube is a max /
//   min over the coordinates: every lane folds its own, the 64 lane values go through one xor-butterfly (max and min are exact,
//   so their order does not matter), and the row's scalars are made wave-uniform with readfirstlane.
// The random words of a row are Philox4x64-10 of (step, stream id, seed): they depend on nothing else, so a row's bits depend
// on its own start, constraint, stream id and the options alone -- not on its batch, its position or the device count.
// Every product and sum of the proposal is a separately rounded multiply or add: contraction to FMA is switched off for this whole
// file (hipcc contracts by default, and HIP's __dmul_rn / __dadd_rn are plain operators that it contracts all the same), so
// that numpy restates a trajectory exactly (tests/ns_reference.py).  A finished row (status != 0) is carried: its point, its
// logL and its counters stay as they are and its trial row is its own point.
// Under a Gaussian prior (mcalf_set_gauss_prior; a.prior.mu != NULL) the constrained quantity is logL + lnprior, one rounded
// add of the launch's logL and row_lnprior (prior_device.h) of the row the wave holds: the start's in the started kernel, the
// trial's in the step kernel's decide; it is what goes into L.  Without one the code path is the one without the branch.
// Packing (mcalf_set_slice_compact): a row that proposes stamps itself with the step; the pack kernel lists the stamped rows in
// row order (integers only), the gather kernel copies their trial rows together for a logL launch over those alone, and the
// step kernel reads a trial's logL through the row's slot.  No row's bits depend on it.
#include <hip/hip_runtime.h>

#include "ns_args.h"

#pragma clang fp contract(off)

#include "prior_device.h"
#include "wave_row.h"

using namespace mcalf;

__global__ __launch_bounds__(kNsWave) void mcalf_slice_start_kernel(const NsArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)row * a.ndim;
    for (int k = lane; k < a.ndim; k += kNsWave) {
        const double v = a.U0[o + k];
        a.U[o + k] = v;
        a.Y[o + k] = v;
    }
    if (lane == 0) {
        a.status[row] = kNsLive;
        a.nevals[row] = 0;
        a.moves[row] = 0;
        a.dir[row] = -1;
        a.stamp[row] = 0;
    }
}

// A start is bad when an entry lies outside [0, 1] or is NaN, or when L(U0) > Lmin is false (NaN makes it false); it is returned
// as given with the logL the launch gave it.  With nmoves == 0 a good start is finished at once.
__global__ __launch_bounds__(kNsWave) void mcalf_slice_started_kernel(const NsArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)row * a.ndim;
    int bad = 0;
    for (int k = lane; k < a.ndim; k += kNsWave) {
        const double v = a.U0[o + k];
        bad |= outside_unit(v);
    }
    double l = a.LY[row];
    if (a.prior.mu) l = l + row_lnprior(a.prior, a.U0 + o, 1);   // (one rounded add; every lane of the wave is here)
    const bool outside = __any(bad);
    if (lane != 0) return;
    a.L[row] = l;
    if (outside || !(l > a.Lmin[row])) a.status[row] = kNsBadStart;
    else if (a.nmoves == 0) a.status[row] = kNsDone;
}

__global__ __launch_bounds__(kNsWave) void mcalf_slice_step_kernel(const NsArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (__builtin_amdgcn_readfirstlane(a.status[row]) != kNsLive) return;
    const size_t o = (size_t)row * a.ndim, n = (size_t)a.nrows;
    double *x = a.U + o, *y = a.Y + o;
    double tl = a.brk[row], tr = a.brk[n + row];
    int dir = __builtin_amdgcn_readfirstlane(a.dir[row]);
    if (a.decide) {
        double ly = a.LY[a.slot ? a.slot[row] : row];
        if (a.prior.mu) ly = ly + row_lnprior(a.prior, y, 1);  // (LY by slot, the trial row by row)
        if (ly > a.Lmin[row]) {                                // accepted: the trial row stays the row's own point
            for (int k = lane; k < a.ndim; k += kNsWave) x[k] = y[k];
            const int mv = a.moves[row] + 1;
            dir = -1;
            if (lane == 0) {
                a.L[row] = ly;
                a.moves[row] = mv;
                a.dir[row] = -1;
                if (mv == a.nmoves) a.status[row] = kNsDone;
            }
            if (mv == a.nmoves) return;
        } else {                                               // rejected: the bracket shrinks towards t = 0, the current point
            const double t = a.brk[2 * n + row];
            if (t < 0.0) tl = t;
            else tr = t;
        }
    }
    if (!a.propose) return;
    uint64_t w[4];                                             // (key word 1 is 0; words 2 and 3 are reserved)
    philox4x64_10((uint64_t)a.it, a.sid[row], a.seed, 0, w);
    const uint64_t w0 = w[0], w1 = w[1];
    if (dir < 0) {                                             // a new direction: the chord of its line through the cube
        dir = (int)(w0 % (uint64_t)a.ndirs);
        const double* d = a.D + (size_t)dir * a.ndim;
        double lo = -__builtin_inf(), hi = __builtin_inf();
        int any = 0;
        for (int k = lane; k < a.ndim; k += kNsWave) {
            const double dk = d[k];
            if (dk != 0.0) {
                const double xa = (0.0 - x[k]) / dk, xb = (1.0 - x[k]) / dk;
                const double mn = xa < xb ? xa : xb, mx = xa < xb ? xb : xa;
                lo = mn > lo ? mn : lo;
                hi = mx < hi ? mx : hi;
                any = 1;
            }
        }
        if (__any(any)) {
            tl = uniform(wave_max(lo));
            tr = uniform(wave_min(hi));
        } else {
            tl = tr = 0.0;
        }
    }
    const double* d = a.D + (size_t)dir * a.ndim;
    const double xi = (double)(w1 >> 11) * 0x1.0p-53;
    const double t = tl + (tr - tl) * xi;
    for (int k = lane; k < a.ndim; k += kNsWave) {
        const double v = x[k] + t * d[k];
        y[k] = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    }
    if (lane != 0) return;
    a.brk[row] = tl;
    a.brk[n + row] = tr;
    a.brk[2 * n + row] = t;
    a.dir[row] = dir;
    a.nevals[row] += 1;
    a.stamp[row] = a.it;                                        // (the step itself: nothing to clear between steps)
    atomicAdd(a.live, 1u);
}

// The rows that proposed a trial in step `it`, in ascending row order: idx[s] = row, slot[row] = s, *live = their count.  One
// workgroup walks the rows kNsPackBlock at a time: a ballot and a popcount inside a wave, the wave sums through LDS, a running
// base from pass to pass.  Integers only, no atomics: the order is the rows' own.
__global__ __launch_bounds__(kNsPackBlock) void mcalf_slice_pack_kernel(const NsArgs a) {
    constexpr int kWaves = kNsPackBlock / kNsWave;
    __shared__ int wsum[kWaves];
    const int tid = threadIdx.x, lane = tid & (kNsWave - 1), wave = tid / kNsWave;
    int base = 0;
    for (int r0 = 0; r0 < a.nrows; r0 += kNsPackBlock) {       // (nrows <= 0x7fff0000: r0 + tid stays an int)
        const int row = r0 + tid;
        const bool on = row < a.nrows && a.stamp[row] == a.it;
        const unsigned long long m = __ballot(on);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int c = wsum[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (on) {
            const int s = before + __popcll(m & ((1ull << lane) - 1ull));
            a.idx[s] = row;
            a.slot[row] = s;
        }
        base += total;
        __syncthreads();                                       // (wsum is written again by the next pass)
    }
    if (tid == 0) *a.live = (unsigned int)base;
}

// One wave per slot of the launch: the trial row of the slot's chain, and the trial row of row 0 -- a row the unpacked launch
// evaluates all the same -- for the slots past the count, whose logL nobody reads.
__global__ __launch_bounds__(kNsWave) void mcalf_slice_gather_kernel(const NsArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int count = (int)__builtin_amdgcn_readfirstlane((int)*a.live);
    const int row = s < count ? __builtin_amdgcn_readfirstlane(a.idx[s]) : 0;
    const double* y = a.Y + (size_t)row * a.ndim;
    double* yc = a.Yc + (size_t)s * a.ndim;
    for (int k = lane; k < a.ndim; k += kNsWave) yc[k] = y[k];
}

namespace mcalf {
const void* ns_kernel_ptr(NsKernel k) {
    static const void* const table[] = {(const void*)&mcalf_slice_start_kernel, (const void*)&mcalf_slice_started_kernel,
                                        (const void*)&mcalf_slice_step_kernel, (const void*)&mcalf_slice_pack_kernel,
                                        (const void*)&mcalf_slice_gather_kernel};   // in the order of enum NsKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kNsKernelCount, "one entry per NsKernel");
    return table[k];
}
}  // namespace mcalf
