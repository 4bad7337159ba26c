// Fused likelihood kernel (kernels.hip), the line evaluation: one (component, line) added to a thread's eight optical depths,
// and the general Voigt path of the lines outside the fast path's damping range.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"
#include "voigt_device.h"
#include "wave_util.h"

namespace mcalf {

// tau[j] += K H(u_j, y) for the thread's kPpt pixels and one (component,line); `tab` is the line's
// folded table in LDS (coefficients, then the line's threshold -- or its segment-mask word -- and the (A, B) of u = nu A - B).
//
// kPreMask (single-tile spectra behind a set-up kernel or a streaming set-up phase): the set-up has classified the
// line's 64 segments already (segment_masks) and the word W sits where the threshold does otherwise.  Pixels and
// nodes are then owned DIFFERENTLY: wave `wv` still evaluates the pixels of segments wv, wv + 8, .. (interleaved, which
// balances the direct work over the waves) -- byte wv of W, bit j = its slot j is interpolated -- but holds the nodes
// of the ADJACENT segments 8 wv .. 8 wv + 7 -- bits 8 i of W >> wv.  A line's core and near wings cover a few adjacent
// segments: the wing zones of the node pass, and often the node pass itself, then concern one or two waves per line
// instead of nearly all of them, and no wave computes a mask.
template <bool kPreMask>
__device__ __forceinline__ void eval_line(const double* __restrict__ tab,
                                          const double (&nu)[kPpt], double (&tau)[kPpt], double nuNode,
                                          double& farNode, unsigned long long segOk, int wv) {
    const double A = tab[kLineLds + 1], B = tab[kLineLds + 2];
    double cF[VT_FDEG + 1];
#pragma unroll
    for (int k = 0; k <= VT_FDEG; ++k) cF[k] = tab[kZFLds + k];
    // The node arithmetic of a wave whose node mask `done` (bit 8 j: segment j of the wave's nodes is interpolated)
    // is not empty.
    auto node_pass = [&](unsigned long long done, double x2n, double t) {
        // byte j -> 0xFF: one bit per lane.  On 32-bit halves (no carry can cross: 0x01010101 * 0xFF = 0xFFFFFFFF),
        // which is two scalar multiplies instead of a 64-bit one.
        const unsigned long long lanes = ((unsigned long long)((unsigned)(done >> 32) * 0xFFu) << 32) | ((unsigned)done * 0xFFu);
        const bool mine = __builtin_amdgcn_inverse_ballot_w64(lanes);   // the scalar mask IS the lane predicate
        double P;
        if (!mine || x2n >= kX2Far) {                         // (lanes of directly evaluated segments never need a wing zone)
            P = cF[VT_FDEG];
#pragma unroll
            for (int k = VT_FDEG - 1; k >= 0; --k) P = fma(P, t, cF[k]);
        } else {
            const bool z0 = x2n >= kX2Wing;
            const double sv = z0 ? t : fma(t, VT_Z1_A, VT_Z1_B);
            const double* cw = tab + (z0 ? kZ0Lds : VT_Z1_OFF);
            P = cw[VT_WDEG];
#pragma unroll
            for (int k = VT_WDEG - 1; k >= 0; --k) P = fma(P, sv, cw[k]);
        }
        fmac_inplace(farNode, mine ? t : 0.0, P);
    };
    // Node pass.  Lane l holds node (l & 7) of the wave's segment (l >> 3).  A segment whose eight
    // nodes (both end pixels included, u monotonic along it) all have u >= uthr, or all u <= -uthr,
    // is wing (|u| >= x_c: no exp(-u^2)) for this line everywhere: its contribution is evaluated at the nodes only and
    // interpolated to the 64 pixels once, after the component loop.  `done` has bit 8 j set when
    // segment j was handled that way.
    unsigned long long done = 0;
    unsigned pix = 0;                                         // kPreMask: bit j = the wave's PIXEL slot j is interpolated
    if (kFarInterp && kPreMask) {
        const unsigned long long W = uniform64(__builtin_bit_cast(unsigned long long, tab[kLineLds]));
        pix = (unsigned)(W >> (8 * wv)) & 0xFFu;
        const unsigned long long nodes = (W >> wv) & 0x0101010101010101ull;
        if (nodes != 0) {                                     // wave-uniform
            const double un = fma(nuNode, A, -B);
            const double x2n = un * un;
            node_pass(nodes, x2n, fast_rcp(fmax(x2n, 4.0)));  // (the same operations on the same operands as below)
        }
    } else if (kFarInterp) {
        const double uthr = tab[kLineLds];
        const double un = fma(nuNode, A, -B);
        // issued ahead of the scalar mask chain below, which then runs in the shadow of the reciprocal
        const double x2n = un * un;
        // lanes outside `mine` only need to stay finite (mine lanes have x2n >= uthr^2 >= 36; 4.0 is an inline
        // constant, 36.0 costs two scalar moves per line)
        const double t = fast_rcp(fmax(x2n, 4.0));
        unsigned long long mp = __builtin_amdgcn_ballot_w64(un >= uthr);
        unsigned long long mn = __builtin_amdgcn_ballot_w64(un <= -uthr);
        // u is monotonic along a segment (segOk excludes the wrapped ones), so its two END nodes -- lanes 8j
        // and 8j+7, the segment's first and last pixel -- decide for all eight.
        mp &= mp >> 7;                                        // bit 8j = first and last node
        mn &= mn >> 7;
        done = uniform64((mp | mn) & segOk);                 // (segOk carries bits 8j only, so `done` does too)
        if (done != 0) node_pass(done, x2n, t);               // wave-uniform
    }
    // Tested on 32-bit halves (one s_bitcmp1_b32 + branch per segment), four segments at a time first: a line's
    // core covers one or two ADJACENT segments of a wave, so one half of the eight is usually interpolated throughout.
    const unsigned doneLo = (unsigned)done, doneHi = (unsigned)(done >> 32);
#pragma unroll
    for (int h = 0; h < kPpt / 4; ++h) {
    const unsigned dh = h ? doneHi : doneLo;
    if (kPreMask ? ((pix >> (4 * h)) & 0xFu) == 0xFu : dh == 0x01010101u) continue;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int j = 4 * h + jj;
        // whole segment interpolated (wave-uniform, the usual case)
        if (__builtin_expect((kPreMask ? (pix >> j) & 1u : (dh >> (8 * jj)) & 1u) != 0u, 1)) continue;
        const double u = fma(nu[j], A, -B);
        const double x2 = u * u;
        // Every branch leaves (t, P) with contribution t * P, and the running optical depth is updated at ONE
        // place after the branches merge: an update inside each branch makes the compiler copy tau[j] into a
        // scratch pair and back (3 vector moves per evaluation).
        double t, P;
        if (x2 >= kX2Far) {                           // |u| >= 16
            t = fast_rcp(x2);
            P = cF[VT_FDEG];
#pragma unroll
            for (int k = VT_FDEG - 1; k >= 0; --k) P = fma(P, t, cF[k]);
        } else if (x2 >= kX2Wing) {                   // 8 <= |u| < 16: polynomial in 1/u^2 (broadcast reads)
            t = fast_rcp(x2);
            const double* cw = tab + kZ0Lds;
            P = cw[VT_WDEG];
#pragma unroll
            for (int k = VT_WDEG - 1; k >= 0; --k) P = fma(P, t, cw[k]);
        } else {                                      // |u| < 8: core table (per-lane LDS gather).  It is valid up to 8, so the
                                                      // pixels between x_c and 8 come here too instead of splitting the wave over
                                                      // a third path (zone 1 serves the interpolation nodes only)
            // |u| < 8 here (NaN converts to 0), so the interval index needs no clamp; s = 8|u| - (2j+1) from 4|u|
            // with the inline constant 2.0 (same value bit for bit, 8.0 costs two scalar moves per segment)
            const double x4 = fabs(u) * 4.0;
            const int jx = (int)x4;
            const double sv = fma(x4, 2.0, -(double)(2 * jx + 1));
            const double* cc = tab + jx * VT_CSTRIDE;
            P = cc[VT_CDEG];
#pragma unroll
            for (int k = VT_CDEG - 1; k >= 0; --k) P = fma(P, sv, cc[k]);
            t = 1.0;                                  // tau += 1 * P rounds exactly like tau += P
        }
        fmac_inplace(tau[j], t, P);
    }
    }
}

// Lines outside the fast path's damping range (flag != 0; none for physical resonance lines).  Kept out
// of the hot loop: the call to the non-inlined general Voigt routine would otherwise pin the running
// optical depths in callee-saved registers and cost a register shuffle per line.
__device__ __forceinline__ void eval_general_lines(const double* __restrict__ sRec, int ncl, const double (&nu)[kPpt],
                                                double (&tau)[kPpt]) {
    for (int cl = 0; cl < ncl; ++cl) {
        const double* rec = sRec + cl * kRecStride;
        if (rec[6] == 0.0) continue;
        const double A = rec[0], B = rec[1], y = rec[2], K = rec[6];
#pragma unroll 1
        for (int j = 0; j < kPpt; ++j) {
            const double u = fma(nu[j], A, -B);
            tau[j] = fma(K, hjert_general(fabs(u), y), tau[j]);
        }
    }
}

}  // namespace mcalf
