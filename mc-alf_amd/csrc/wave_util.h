// Fused likelihood kernel (kernels.hip), stage 0: what a wave or a workgroup does with its registers -- the XCD it runs on, tile
// positions, the DPP sums, values the compiler is told are wave-uniform, lane reads, accumulators tied to their register.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"

namespace mcalf {

// The XCD a wave runs on (XCC_ID, bits 3:0 of hardware register 20 on gfx942 / gfx950): all four bits for the context's
// probe (mcalf_xcd_probe_kernel), three for the streaming launch -- the host only takes that launch on a stream whose
// workgroups the probe saw on exactly the XCDs 0 .. 7 of an unpartitioned MI355X (host_stream.cpp), and checks after every
// launch that each of them did receive workgroups (status[2]).
__device__ __forceinline__ int xcd_raw() { return (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15); }
__device__ __forceinline__ int xcd_id() { return (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & (kXcds - 1)); }

__device__ __forceinline__ int tile_pos(int i) { return (i & 7) * kPlaneStride + (i >> 3); }

// Value of lane (l - N) within each row of 16 lanes (0 where there is none): one v_mov_b32_dpp per half,
// no LDS round trip (ds_bpermute, which __shfl_* compiles to, costs an LDS latency per step).
template <int kCtrl, int kRowMask = 0xF>
__device__ __forceinline__ double dpp_move(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, kCtrl, kRowMask, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), kCtrl, kRowMask, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// Sum over the 64 lanes of a wave; the total ends up in lane 63 (DPP row shifts + row broadcasts).
__device__ __forceinline__ double wave_sum_to_last(double v) {
    v += dpp_move<0x111>(v);          // row_shr:1
    v += dpp_move<0x112>(v);          // row_shr:2
    v += dpp_move<0x114>(v);          // row_shr:4
    v += dpp_move<0x118>(v);          // row_shr:8   -> lane 15 of every row holds the row sum
    v += dpp_move<0x142, 0xA>(v);     // row_bcast:15 into rows 1 and 3
    v += dpp_move<0x143, 0xC>(v);     // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave sum
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Tell the compiler a 64-bit value is wave-uniform (keeps it in SGPRs, branches on it are scalar).
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Sum over the 64 lanes of a wave, result in every lane (as a wave-uniform value): the DPP reduction above and
// one v_readlane per half -- no LDS round trips (a __shfl_xor butterfly is 12 ds_bpermute, each an LDS latency
// on the serial path of the set-up kernel).
__device__ __forceinline__ double wave_allsum(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, wave_sum_to_last(v));
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, 63), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Sum over the workgroup, result in every thread; fixed order (deterministic).
__device__ __forceinline__ double block_sum(double v, double* scratch, int tid) {
    v = wave_sum(v);
    if ((tid & 63) == 0) scratch[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += scratch[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ double finalize_value(int mode, double sum, double nnz, bool asymm, double c4,
                                                 double c5, double veto4, double veto5) {
    if (mode == kModeChi2) return (nnz == 0.0) ? INFINITY : sum;   // hires_fitter.py:241-246
    if (asymm && (c5 > veto5 || c4 > veto4)) return -INFINITY;     // :296-303
    return -0.5 * sum;                                             // :294
}

// acc += a * b and acc += a with the accumulator tied to its register: without the tie the compiler
// gives every update of the thread's 8 running optical depths a fresh register and copies all of them
// back at the loop back-edge (16 v_mov_b64 per line).
__device__ __forceinline__ void fmac_inplace(double& acc, double a, double b) {
    asm("v_fmac_f64 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void add_inplace(double& acc, double a) {
    asm("v_add_f64 %0, %0, %1" : "+v"(acc) : "v"(a));
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, lane), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

}  // namespace mcalf
