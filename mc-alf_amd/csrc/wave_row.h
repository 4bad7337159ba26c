// Device helpers of the kernels that give ONE wave64 to a row: lane k owns coordinates k, k + 64, ...; a row's scalars are
// folded over the lanes by one fixed xor-butterfly and made wave-uniform with readfirstlane; the random words of a row are
// Philox4x64-10 blocks.  (A kernel that gives a row several waves may take wave_sum alone, for its waves' partials.)
// The only floating-point arithmetic in here is wave_sum's add, which has no product to contract with: it does not matter
// whether the including file has switched contraction to FMA off before it includes this (the samplers' files do) or has
// left it on.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcalf {

// A value every lane already holds with the same bits, as a wave-uniform (scalar) one.
__device__ __forceinline__ double uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Sum, maximum and minimum over the wave's 64 lanes, the same butterfly every time (every lane gets the result; max and min are
// exact, so their order does not matter).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}

// 1 for a coordinate outside the unit cube [0, 1] or NaN, else 0 (a lane ORs it over its coordinates, a ballot over the lanes).
__device__ __forceinline__ int outside_unit(double v) { return (v >= 0.0 && v <= 1.0) ? 0 : 1; }

// Philox4x64-10 (Salmon et al. 2011), the constants numpy's Philox bit generator uses.
constexpr uint64_t kPhiloxM0 = 0xD2E7470EE14C6C93ull, kPhiloxM1 = 0xCA5A826395121157ull;
constexpr uint64_t kPhiloxW0 = 0x9E3779B97F4A7C15ull, kPhiloxW1 = 0xBB67AE8584CAA73Bull;

// The block of counter (c0, c1, c2, 0) under key (k0, k1): its four words.
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t k0, uint64_t k1, uint64_t (&w)[4]) {
    uint64_t c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t hi0 = __umul64hi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint64_t hi1 = __umul64hi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// The block of counter (c0, 0, c2, 0).
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c2, uint64_t k0, uint64_t k1, uint64_t (&w)[4]) {
    philox4x64_10(c0, 0, c2, k0, k1, w);
}

}  // namespace mcalf
