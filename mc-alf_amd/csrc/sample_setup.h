// Fused likelihood kernel (kernels.hip), the set-up of a live point by one wave: its (component, line) records, their
// segment-mask words, the LSF taps and the header; and the hand-out order of a batch.  The set-up kernel, the streaming
// launch's set-up phase and the one-launch variant all run setup_sample(), so that they give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"
#include "voigt_device.h"
#include "wave_util.h"

namespace mcalf {

// 10^x as exp(x ln 10) with the product carried in two doubles (about 1 ulp, a fraction of the cost of pow()).
__device__ __noinline__ double pow10_edge(double x) { return pow(10.0, x); }   // +-inf, NaN, over/underflow (10**-inf = 0)
__device__ __forceinline__ double pow10_fast(double x) {
    constexpr double kLn10Hi = 2.302585092994045901, kLn10Lo = -2.1707562233822494e-16;
    if (!(fabs(x) <= 300.0)) return pow10_edge(x);       // the library's edge cases, kept out of line
    const double p = x * kLn10Hi;
    const double e = fma(x, kLn10Hi, -p) + x * kLn10Lo;
    const double r = exp_neg(-p);                        // == exp(p) to the last bit (voigt_device.h), a third of the code
    return fma(r, e, r);
}

// Record per (component,line): [A, B, x2c, y, K, Kyt, Kgen, uthr]   (general-path lines: [A, B, y, 0, 0, 0, K, 0])
//   u = nu*A - B;  tau += K H(u, y);  Kyt = K y / sqrt(pi) scales the wing polynomials;
//   x2c = x_c^2: beyond it exp(-x^2) is below 2e-17 in optical depth, so the line is pure wing there (the
//        interpolation threshold never lies inside it; nodes between x_c and 8 use the zone-1 polynomial);
//   Kgen != 0 -> general path (eval_general_lines);
//   uthr: a 64-pixel segment whose pixels all have |u| >= uthr is evaluated at 8 nodes and interpolated.
__device__ inline void build_line_record(double* rec, double logN, double z, double b_kms, const LineDev& ln,
                                         double dnu_seg) {
    const double cold = pow10_fast(logN);                // :357  10.0**N
    const double zp1 = z + 1.0;                          // :358
    // ONE division per record: 1/dnu = wrest / b (:360 with :376's b*1e5); everything that the reference divides
    // by dnu is a multiple of it (five IEEE divisions were a third of this kernel's serial path; the products
    // differ from the quotients by an ulp, far below the 1e-11 cancellation noise u carries anyway)
    const double rdnu = ln.wrest_cm / (b_kms * 1e5);
    const double a = ln.gamma4pi * rdnu;                 // :361  gamma / (4 pi dnu)
    const double cne = kTauConst * cold * ln.f;          // :364
    const double K = cne * rdnu;                         // :365  tau = cne * H / dnu
    rec[0] = zp1 * rdnu;                                 // u = ((c/(lam/zp1)) - nujk)/dnu  (:362)
    rec[1] = ln.nujk * rdnu;
    rec[2] = core_limit_x2(K);
    rec[3] = a;
    rec[4] = K;
    rec[5] = K * a * kInvSqrtPi;
    double flag = 0.0;
    if (!(a <= kYFastMax) || !(a >= 0.0)) flag = 1.0;    // general path (also NaN)
    else if (K * 1.6e-28 > 2e-17) flag = 1.0;            // absurd columns: exp(-x^2) matters past |x| = 8
    rec[6] = 0.0;
    // interpolation error kInterpC (du/u0)^8 Kyt/u0^2 <= kInterpTol  ->  u0^10 >= kInterpC Kyt du^8 / tol
    const float du = (float)(rec[0] * dnu_seg);
    const float du2 = du * du, du4 = du2 * du2;
    const float q = (float)(kInterpC / kInterpTol) * (float)rec[5] * du4 * du4;
    // q^0.1 as exp2(0.1 log2 q) on the hardware's v_log_f32 / v_exp_f32 (q >= 1, so no denormal case; their ~1e-7
    // relative error is nothing against the margin) -- powf() expands to ~150 instructions of this kernel's serial path
    double uthr = (double)__builtin_amdgcn_exp2f(0.1f * __builtin_amdgcn_logf(fmaxf(q, 1.0f))) * 1.02;   // 2 % margin over the float estimate
    uthr = fmax(uthr, (double)__fsqrt_rn((float)rec[2]) * 1.000001);           // never inside the core table's range (x2c in [36, 64])
    rec[7] = !(uthr < 1e30) ? INFINITY : uthr;
    if (flag != 0.0) {
        // General-path line: the hot loop carries no test for it.  Its fast-path view is a line of zero
        // strength (folded tables all zero, every segment "interpolated"), and eval_general_lines() finds
        // the real damping parameter in slot 2 and the real K in slot 6 (K != 0 marks the record).
        rec[2] = a; rec[3] = 0.0; rec[4] = 0.0; rec[5] = 0.0; rec[6] = K; rec[7] = 0.0;
    }
    // |1+z| beyond 1e100 (or infinite): every |u| overflows, the reference's wofz returns 0 and the line adds
    // nothing (tau < 1e-200).  Written out as a record that contributes exact zeros, because 1/u^2 -> 0 would
    // put 0 * inf = NaN through the reciprocal's Newton step.  NaN parameters still propagate as NaN.
    if (!(fabs(zp1) < 1e100) && zp1 == zp1 && fabs(K) < 1e100 && fabs(a) < 1e100) {
        rec[0] = 0.0; rec[1] = -1e6; rec[2] = 36.0; rec[3] = 0.0; rec[4] = 0.0; rec[5] = 0.0; rec[6] = 0.0;
        rec[7] = 0.0;
    }
}

// theta[i] of one sample: either the row element itself or, with unit-cube input, cube*ptp + min with the
// separately rounded multiply and add numpy performs (hires_fitter.py:206 / :214) and int() on the ncomp slot.
__device__ __forceinline__ double sample_param(const KArgs& a, const double* __restrict__ p, int i) {
    double v = p[i];
    if (a.prior_lo) {
        const double lo = a.prior_lo[i], hi = a.prior_hi[i];
        {
#pragma clang fp contract(off)
            const double scaled = v * (hi - lo);
            v = scaled + lo;
        }
        if (a.prior_int && i == a.startind) v = trunc(v);        // :207-208
    }
    return v;
}

constexpr int kOrderBuckets = 64;       // component counts 0 .. 62 get a bucket each, larger ones share the last
constexpr int kOrderKeys = 16;          // keys a thread of the ordering workgroup holds at a time

// Active components of live point s: int(p[startind]) on the numpy path (:428), floor on the JAX path (:616),
// clamped to [0, ncompmax].
template <bool kZeroPad>
__device__ __forceinline__ int sample_ncomp(const KArgs& a, long s) {
    const double ncv = sample_param(a, a.P + (size_t)s * a.ndim, a.startind);
    const double nct = kZeroPad ? floor(ncv) : trunc(ncv);
    return (nct >= 1.0) ? ((nct >= (double)a.ncompmax) ? a.ncompmax : (int)nct) : 0;
}

// One workgroup of the set-up kernel: counting sort of the live points by component count, most components
// first, into a.order.  The fused kernel's queue then hands out similar work items next to each other (the two
// workgroups that share a CU run evenly matched items: measured -2.4 % kernel time at config C with rows
// sorted on the host) and the shortest items last.  LDS atomics only; the order inside a bucket is whatever the
// atomics give, which changes who evaluates a live point, never its value.
template <bool kZeroPad>
__device__ void build_order(const KArgs& a, long batch) {
    __shared__ int hist[kOrderBuckets];
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid < kOrderBuckets) hist[tid] = 0;
    __syncthreads();
    const long chunk = (long)kOrderKeys * nthr;
    auto load_keys = [&](long base, int (&key)[kOrderKeys]) {
#pragma unroll
        for (int k = 0; k < kOrderKeys; ++k) {                     // independent loads: one memory round trip per chunk
            const long s = base + (long)k * nthr + tid;
            key[k] = (s < batch) ? min(a.ncompmax - sample_ncomp<kZeroPad>(a, s), kOrderBuckets - 1) : -1;
        }
    };
    int key[kOrderKeys];
    // pass 1: bucket counts
    for (long base = 0; base < batch; base += chunk) {
        load_keys(base, key);
#pragma unroll
        for (int k = 0; k < kOrderKeys; ++k)
            if (key[k] >= 0) atomicAdd(&hist[key[k]], 1);
    }
    __syncthreads();
    // counts -> first position of each bucket: exclusive prefix sum over the 64 buckets by one wave
    if (tid < 64) {
        static_assert(kOrderBuckets == 64, "one bucket per lane");
        const int c = hist[tid];
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (tid >= off) incl += up;
        }
        hist[tid] = incl - c;
    }
    __syncthreads();
    // pass 2: positions.  A batch of one chunk (4096 live points with 256 threads) still holds its keys.
    for (long base = 0; base < batch; base += chunk) {
        if (batch > chunk) load_keys(base, key);
#pragma unroll
        for (int k = 0; k < kOrderKeys; ++k)
            if (key[k] >= 0) a.order[atomicAdd(&hist[key[k]], 1)] = (int)(base + (long)k * nthr + tid);
    }
}

// Segment-mask words of the records a wave holds one per lane (`have`: the lanes whose record is in use), for
// eval_line<true>: bit 8 i + v of a record's word is set when segment 8 v + i of the (single) tile is interpolated
// for that line -- both end pixels at u >= uthr or both at u <= -uthr, with eval_line's own fma and comparisons on the
// values its node lanes 0 and 7 load, so the classification is the one-launch variant's bit for bit -- and the
// context allows it (segok).  Lane l tests segment 8 (l & 7) + (l >> 3) of one record at a time -- nuLo / nuHi are that
// segment's first and last pixel frequency, okW the lanes whose segment may be interpolated -- so that the ballots ARE
// the word.  All 64 lanes must be active.  uthr = 0 (general-path and zero-strength records) gives every allowed
// segment, uthr = inf or NaN none, as the comparisons do in the loop.
__device__ __forceinline__ double segment_masks(const double (&rec)[kRecStride], int lane, unsigned long long have, double nuLo,
                                                double nuHi, unsigned long long okW) {
    unsigned long long word = 0;
    for (unsigned long long todo = have; todo != 0; todo &= todo - 1) {       // (wave-uniform)
        const int r = __builtin_ctzll(todo);
        const double A = readlane_f64(rec[0], r), B = readlane_f64(rec[1], r), uthr = readlane_f64(rec[7], r);
        const double u0 = seg_u(nuLo, A, B), u1 = seg_u(nuHi, A, B);
        const unsigned long long mp = __builtin_amdgcn_ballot_w64(seg_above(u0, uthr)) & __builtin_amdgcn_ballot_w64(seg_above(u1, uthr));
        const unsigned long long mn = __builtin_amdgcn_ballot_w64(seg_below(u0, uthr)) & __builtin_amdgcn_ballot_w64(seg_below(u1, uthr));
        const unsigned long long w = (mp | mn) & okW;
        if (lane == r) word = w;
    }
    return __builtin_bit_cast(double, word);
}

// A wave's table of segment-end frequencies in LDS (kSegEnds doubles of its own: entry 2 m / 2 m + 1 = first / last pixel
// frequency of segment m), which the records' searches then read lane by lane (seg_word_search) -- two loads a lane, the
// same two the walk needs.  Written and read by the one wave: no workgroup barrier.  All 64 lanes must be active.
__device__ __forceinline__ void fill_segment_ends(const KArgs& a, int lane, double* ends) {
    static_assert(kSegEnds == 128, "two ends per lane");
    const double e0 = a.nu[seg_end_pixel(lane)], e1 = a.nu[seg_end_pixel(lane + 64)];
    ends[lane] = e0; ends[lane + 64] = e1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The set-up of live point s by ONE wave (`lane` = 0..63): decode, records, taps, header, written through the given
// pointers -- the context's workspaces in HBM (mcalf_sample_kernel) or the workgroup's own LDS (the one-launch
// variant of the fused kernel that small calls use).  One body, so both give the same bits.
// segMasks: the records carry their segment-mask word in slot 7 instead of the threshold (the set-up kernel and the
// streaming set-up phase of single-tile contexts, whose fused kernel is eval_line<true>); the one-launch variant, the
// resident kernel and tiled contexts leave the threshold there and compute nothing more.  `ends` is then the wave's table
// of segment ends (fill_segment_ends).  Every lane finds the word of ITS record by boundary search (seg_word_search: the
// same fma and comparisons at 16 of the 128 ends) where mcalf_create found the context's ends monotone (a.seg_search,
// wave-uniform); otherwise the walk over all of them stays in force (segment_masks).
template <bool kZeroPad>
__device__ __forceinline__ void setup_sample(const KArgs& a, long s, int lane, double* recs, double* taps, bool writeTaps,
                                             SampleHdr* hdrOut, bool writeTheta, bool segMasks, const double* ends = nullptr) {
    const int rowlen = (a.mode == kModeOneComp) ? 5 : a.ndim;
    const double* p = a.P + (size_t)s * rowlen;
    const bool walk = segMasks && a.seg_search == 0;
    // (the walk: lane l tests segment mseg of one record at a time)
    const int mseg = 8 * (lane & 7) + (lane >> 3);
    double nuLo = 0.0, nuHi = 0.0;
    unsigned long long tileOk = 0;
    if (segMasks) tileOk = a.segok[0];
    if (walk) { nuLo = ends[2 * mseg]; nuHi = ends[2 * mseg + 1]; }
    // ---- 1. decode the parameter vector ---------------------------------------------------
    double R, cont;
    int nc, nfill_eff;
    if (a.mode == kModeOneComp) {                       // hires_fitter.py:379-406
        R = p[0];
        cont = p[1];
        nc = 1;
        nfill_eff = 0;
    } else {
        R = a.freespecres ? sample_param(a, p, 0) : a.specres_fixed;     // :412-417
        cont = a.freecont ? sample_param(a, p, a.freespecres ? 1 : 0) : a.contval_fixed;   // :419-425
        const double ncv = sample_param(a, p, a.startind);
        if (a.theta_out && writeTheta)
            for (int i = lane; i < a.ndim; i += 64) a.theta_out[(size_t)s * a.ndim + i] = sample_param(a, p, i);
        // numpy path: int() truncates (:428); JAX path: floor (:616)
        const double nct = kZeroPad ? floor(ncv) : trunc(ncv);
        nc = (nct >= 1.0) ? ((nct >= (double)a.ncompmax) ? a.ncompmax : (int)nct) : 0;
        nfill_eff = a.targonly ? 0 : a.nfill;           // :437
    }
    // onecomp_fill: 0 = every line of the component, 1 = the filler line, 2 + k = line k alone
    const int nl_eff = (a.mode == kModeOneComp && a.onecomp_fill) ? 1 : a.nlines;
    const int ncl = nc * nl_eff + nfill_eff;

    // One slot per POSSIBLE (component, line) and filler, so that every load below is independent of the
    // sample's ncomp (one memory round trip); the record lands at its compacted index afterwards.
    const int nTargetSlots = (a.mode == kModeOneComp) ? nl_eff : a.ncompmax * a.nlines;
    const int nSlots = nTargetSlots + ((a.mode == kModeOneComp) ? 0 : a.nfill);
    int ngenLane = 0;
    // (the walk: whole rounds of 64 -- the lanes past the last slot repeat it, write nothing and serve the ballots)
    const int nSlotsRun = walk ? (nSlots + 63) & ~63 : nSlots;
    for (int slot0 = lane; slot0 < nSlotsRun; slot0 += 64) {
        const bool spare = walk && slot0 >= nSlots;
        const int slot = spare ? nSlots - 1 : slot0;
        double logN, z, b;
        const LineDev* ln;
        int dst;                                    // index in the compacted record list, -1: inactive
        if (a.mode == kModeOneComp) {
            logN = p[2]; z = p[3]; b = p[4];
            ln = (a.onecomp_fill == 0) ? (a.lines + slot)
               : (a.onecomp_fill == 1) ? (a.lines + a.nlines) : (a.lines + (a.onecomp_fill - 2));
            dst = slot;
        } else if (slot < nTargetSlots) {
            const int c = slot / a.nlines;
            const int l = slot - c * a.nlines;
            const int q = 1 + 3 * c + a.startind;               // :431  (N, z, b)
            logN = sample_param(a, p, q); z = sample_param(a, p, q + 1); b = sample_param(a, p, q + 2);
            ln = a.lines + l;
            dst = (c < nc) ? slot : -1;                         // components >= int(p[startind]) are skipped (:430)
        } else {
            const int k = slot - nTargetSlots;
            const int q = 3 * k + a.endind;                     // :439
            logN = sample_param(a, p, q); z = sample_param(a, p, q + 1); b = sample_param(a, p, q + 2);
            ln = a.lines + a.nlines;
            dst = (nfill_eff > 0) ? nc * a.nlines + k : -1;
        }
        if (spare) dst = -1;
        double rec[kRecStride];
        build_line_record(rec, logN, z, b, *ln, a.dnu_seg);
        if (walk)
            rec[7] = segment_masks(rec, lane, __builtin_amdgcn_ballot_w64(dst >= 0), nuLo, nuHi,
                                   __builtin_amdgcn_ballot_w64(((tileOk >> mseg) & 1ULL) != 0));
        else if (segMasks)
            rec[7] = __builtin_bit_cast(double, (unsigned long long)seg_word_search(rec[0], rec[1], rec[7], ends, a.seg_search, tileOk));
        ngenLane += __popcll(__ballot(dst >= 0 && rec[6] != 0.0));        // (wave-uniform count)
        if (dst >= 0) {
#pragma unroll
            for (int k = 0; k < kRecStride; ++k) recs[dst * kRecStride + k] = rec[k];
        }
    }

    // ---- LSF taps --------------------------------------------------------------------------
    int n;          // half-width in pixels
    bool bad = false;
    const double sigma = (R / kFwhmToSigma) / a.velstep;        // :454 / :667
    if (kZeroPad) {
        n = a.jax_half;                                         // :549-560 fixed grid
    } else if (R > a.velstep) {                                 // :445
        const double nd = ceil(kKernelReach * sigma);           // :458
        if (!(nd <= (double)a.n_cap)) { bad = true; n = 0; }
        else n = (int)nd;                                       // x_size = int(2n)+1  (:459)
    } else {
        n = 0;
    }
    // Every wave computes the (few) taps itself, so the normalisation needs no workgroup barrier;
    // wave 0 writes them.  astropy normalises the kernel by its sum and its C loop then divides by
    // the tap sum it accumulates next to the data sum (`bot`); the JAX path only normalises (:670).
    const int ntap8 = (2 * n + 1 + 7) & ~7;
    const double inv2s2 = kZeroPad ? 1.0 / (2.0 * sigma * sigma) : 0.5 / (sigma * sigma);
    const double amp = kZeroPad ? 1.0 : 1.0 / (sqrt(2.0 * M_PI) * sigma);          // Gaussian1DKernel amplitude
    double wsum = 0.0, botOrdered = 0.0;
    if (ntap8 <= 64) {                               // the usual case: one tap per lane, one exp
        const double dk = (double)(lane - n);
        const double g = (lane > 2 * n) ? 0.0 : ((n == 0 && !kZeroPad) ? 1.0 : exp_neg((dk * dk) * inv2s2) * amp);
        const double gsum = wave_allsum(g);
        wsum = g / gsum;
        if (lane < ntap8 && writeTaps) taps[lane] = wsum;
        // astropy's loop adds the taps up next to the data sum, tap after tap (`bot`), and divides by that: formed
        // here in the SAME order as the fused kernel's numerator chain (tap 0 first), so that a constant model comes
        // out of the convolution as exactly that constant, as it does in the reference (hires_fitter.py:463-464)
        // (unrolled over the 64 lanes with constant lane numbers, a scalar trip count and an early exit: as a counted loop
        // over the per-lane n it ran under exec masks with a vector compare per step, 2.4 us on the set-up kernel)
        if (!kZeroPad) {
            const unsigned long long wb = __builtin_bit_cast(unsigned long long, wsum);
            const int last = __builtin_amdgcn_readfirstlane(2 * n);      // (the same in every lane: say so, or the loop runs under exec masks)
#pragma unroll
            for (int k = 0; k < 64; ++k) {                   // (no `break`: a constant trip count is what lets it unroll)
                if (k <= last) {
                    const unsigned lo = __builtin_amdgcn_readlane((unsigned)wb, k), hi = __builtin_amdgcn_readlane((unsigned)(wb >> 32), k);
                    botOrdered += __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
                }
            }
        }
    } else {
        double gsum = 0.0;
        for (int k = lane; k <= 2 * n; k += 64) {
            const double dk = (double)(k - n);
            gsum += exp_neg((dk * dk) * inv2s2) * amp;                                  // :669 / Gaussian1D
        }
        gsum = wave_allsum(gsum);
        for (int k = lane; k < ntap8; k += 64) {
            const double dk = (double)(k - n);
            const double w = (k <= 2 * n) ? exp_neg((dk * dk) * inv2s2) * amp / gsum : 0.0;   // zero-padded to 8
            if (writeTaps) taps[k] = w;
        }
        // (more than 64 taps: rare; every lane repeats the tap expression for the tap-ordered sum)
        if (!kZeroPad)
            for (int k = 0; k <= 2 * n; ++k) {
                const double dk = (double)(k - n);
                botOrdered += exp_neg((dk * dk) * inv2s2) * amp / gsum;
            }
    }
    const double bot = kZeroPad ? 1.0 : botOrdered;
    const int ngen = ngenLane;
    if (lane == 0) {
        SampleHdr h;
        h.cont = cont; h.bot = bot; h.ncl = ncl; h.n = n; h.bad = bad ? 1 : 0; h.ngeneral = ngen;
        *hdrOut = h;
    }
}

}  // namespace mcalf
