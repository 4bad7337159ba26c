// The optical-depth kinematics kernels for gfx950, float64 (mcalf_kinematics_batch): per row and target line the integral of
// the model's optical depth over the spectrum, its centroid, its width and the wavelengths below which given fractions of it lie.
//
//     tau[k]   = sum_{c < nc} tau_cl(wl[k])                  slots in slot order, one accumulator from 0.0
//     t[k]     = tau[k] dlam[k]
//     S[k]     = sum_{j <= k} t[j],   I = S[npix - 1]
//     lam_mean = piv + (sum t[k] (wl[k] - piv)) / I,   piv = wl[npix / 2]
//     lam_rms  = sqrt( (sum t[k] (wl[k] - lam_mean)^2) / I )
//     lam_q    = e[k+1] - (e[k+1] - e[k]) clamp((S[k] - q I) / t[k], 0, 1),   k the first pixel with !(S[k] < q I)
//
// tau is the equivalent widths' (tau_fold.h, hjert_general, the records of mcalf_eqw_setup_kernel under the layout's
// indexing).  Nothing is convolved, the continuum does not enter, fillers take no part.
//
//   sums      workgroup = (row, tile of kKinTile pixels), lines outer, slots inner, as the equivalent widths' pixel kernel.  Per
//             line and SLAB (the 64 consecutive pixels of one wave at one j) the inclusive scan of t over the lanes; lane 63's
//             value is the slab's sum of t.  A thread adds its t (wl - piv) in pixel order; the wave's 64 sums go through the
//             fixed butterfly, once per line.
//   offsets   one thread per (row, line): the slabs in pixel order, each slab's sum replaced by the sum of those before it;
//             what is left after the last slab is I.  Then lam_mean and the targets q[j] I.
//   scan      the sums pass again (the same inlined code: t has the same bits), S[k] = offset of the slab + the scan inside
//             it -- so the S of a slab's last pixel IS the next slab's offset, and S[npix - 1] is I.  Per quantile a ballot
//             of !(S < target); the first set lane of a wave's first such slab is the wave's candidate.  The targets are
//             wave-uniform.  The wave's sum of t (wl - lam_mean)^2 as the sums pass formed its first moment.  nq = 0: no scan.
//   finalize  one thread per (row, line): per quantile the candidate with the smallest pixel index over the tiles' waves (the
//             first pixel of the definition, whatever the rounding of S does), the interpolation between the cell's edges,
//             the squares' waves in order, the NaN rules.
// T is recomputed by the scan pass, not stored: a [rows][nlines][npix] workspace would cost a write and a read of 8 bytes per
// pixel and line to save a Voigt pass whose tables are already in LDS, and would cut the rows of a pass by an order of magnitude.
// No atomics and one summation order: a row's bits do not depend on its batch, its position, its pass, nq, the values of q, the
// outputs requested or the device.
#include <hip/hip_runtime.h>

#include "kin_args.h"
#include "tau_fold.h"
#include "voigt_device.h"
#include "wave_row.h"

// Every product and sum below is a separately rounded multiply or add (hipcc contracts by default): the two pixel passes must
// form t, and what they add up, with the same bits.  The Voigt code of the headers above keeps its own explicit fma.
#pragma clang fp contract(off)

using namespace mcalf;

namespace {

__device__ __forceinline__ int kin_nrec(const KinArgs& a) { return a.lay.ncompmax * a.lay.nlines; }
__device__ __forceinline__ int kin_nslabs(const KinArgs& a) { return a.ntiles * kKinSlabs; }

// v of the lane `ctrl` names (a DPP control: row_shr:n, row_bcast:15, row_bcast:31) inside the rows of `rows` (a row is 16 lanes),
// 0.0 in every lane that has no such source or whose row is not in `rows`.  Two 32-bit DPP moves on the vector pipe.
template <int kCtrl, int kRows>
__device__ __forceinline__ double dpp_or_zero(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, kCtrl, kRows, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), kCtrl, kRows, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Inclusive scan of v over the wave's 64 lanes in lane order, six fixed steps: inside every row of 16 lanes the shifts by 1, 2, 4
// and 8, then row 0's and row 2's totals onto rows 1 and 3, then the first half's total onto rows 2 and 3.  Lane 63 ends with
// the wave's sum.  (The same steps through __shfl_up are twelve LDS-pipe permutes per scan instead of twelve vector moves.)
__device__ __forceinline__ double wave_scan(double v) {
    v += dpp_or_zero<0x111, 0xf>(v);                                               // row_shr:1
    v += dpp_or_zero<0x112, 0xf>(v);                                               // row_shr:2
    v += dpp_or_zero<0x114, 0xf>(v);                                               // row_shr:4
    v += dpp_or_zero<0x118, 0xf>(v);                                               // row_shr:8
    v += dpp_or_zero<0x142, 0xa>(v);                                               // row_bcast:15 into rows 1 and 3
    v += dpp_or_zero<0x143, 0xc>(v);                                               // row_bcast:31 into rows 2 and 3
    return v;
}

// The pixel pass.  kScan = false: the sums pass; true: the scan pass.
template <bool kScan>
__device__ __forceinline__ void kin_pixel(const KinArgs& a, double (&sTab)[2][kFoldTab]) {
    const int r = blockIdx.y, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    double T0[VT_NY], T1[VT_NY];
    fold_load<kKinBlock>(a.tabs, t, T0, T1);
    double nu[kKinPpt];                        // (dlam and wl are read per line, after the slots: they are not live across the Voigt pass)
#pragma unroll
    for (int j = 0; j < kKinPpt; ++j) nu[j] = a.nu[min((int)blockIdx.x * kKinTile + j * kKinBlock + t, a.npix - 1)];
    const int nrec = kin_nrec(a), nslabs = kin_nslabs(a), nwaves = a.ntiles * kKinWaves;
    const double* recs = a.recs + (size_t)r * nrec * kEqwRec;
    const double piv = a.wl[a.npix >> 1];
    int buf = 0;
    for (int l = 0; l < a.lay.nlines; ++l) {
        double st[kKinPpt];                                                        // running sum of tau over the slots, per pixel
#pragma unroll
        for (int j = 0; j < kKinPpt; ++j) st[j] = 0.0;
        for (int c = 0; c < a.lay.ncompmax; ++c) {
            const double* rec = recs + (size_t)(c * a.lay.nlines + l) * kEqwRec;
            const int kind = __builtin_amdgcn_readfirstlane((int)rec[5]);          // the same for the whole workgroup: a scalar branch
            if (kind != (int)kEqwFast && kind != (int)kEqwGeneral) continue;
            const double A = rec[0], B = rec[1], y = rec[2], K = rec[3];
            if (kind == (int)kEqwFast) {
                double* tab = sTab[buf];
                fold_store<kKinBlock>(tab, T0, T1, t, y, K, rec[4]);
                __syncthreads();                                                   // (the other table is still being read by slower waves)
                buf ^= 1;
#pragma unroll
                for (int j = 0; j < kKinPpt; ++j) st[j] += tau_fast(tab, fma(nu[j], A, -B));
            } else {
#pragma unroll
                for (int j = 0; j < kKinPpt; ++j) st[j] += K * hjert_general(fabs(fma(nu[j], A, -B)), y);
            }
        }
        const size_t rl = (size_t)r * a.lay.nlines + l;
        double* sumT = a.part + rl * 2 * nslabs;                                   // plane 0, plane 1 behind it
        double* sumX = sumT + nslabs;
        const double* head = a.head + rl * kKinHead;
        const double mean = kScan ? head[1] : 0.0;
        unsigned found = 0;                                                        // bit q: the wave has its candidate for quantile q (wave-uniform)
        double candK = -1.0, candS = 0.0, candT = 0.0;                             // lane q holds quantile q's
        double mom = 0.0;                                                          // the thread's sum_j t_j (wl_j - piv), or t_j (wl_j - lam_mean)^2, in j order
#pragma unroll
        for (int j = 0; j < kKinPpt; ++j) {
            const int i = (int)blockIdx.x * kKinTile + j * kKinBlock + t;
            const bool ok = i < a.npix;
            const double wlj = a.wl[ok ? i : a.npix - 1];
            const double tj = ok ? st[j] * a.dlam[i] : 0.0;
            const int slab = blockIdx.x * kKinSlabs + j * kKinWaves + wave;
            if (!kScan) {
                const double incl = wave_scan(tj);
                if (lane == 63) sumT[slab] = incl;
                mom += tj * (wlj - piv);
            } else {
                const double d = wlj - mean;
                mom += tj * d * d;
                if (a.nq == 0) continue;                                           // S serves the quantiles alone
                const double S = sumT[slab] + wave_scan(tj);
                const int i0 = blockIdx.x * kKinTile + j * kKinBlock + wave * 64;  // the slab's first pixel
                const bool last = i0 + lane == a.npix - 1;                         // "if there is none, k = npix - 1"
                for (int q = 0; q < a.nq; ++q) {
                    if ((found >> q) & 1u) continue;
                    const double target = head[2 + q];
                    const unsigned long long m = __ballot(ok && (!(S < target) || last));
                    if (m == 0) continue;
                    const int first = __ffsll((long long)m) - 1;
                    const double cS = __shfl(S, first, 64), cT = __shfl(tj, first, 64);
                    if (lane == q) {
                        candK = (double)(i0 + first);
                        candS = cS;
                        candT = cT;
                    }
                    found |= 1u << q;
                }
            }
        }
        mom = wave_sum(mom);
        if (lane == 0) sumX[blockIdx.x * kKinWaves + wave] = mom;
        if (kScan && lane < a.nq) {
            double* cd = a.cand + (((rl * nwaves + blockIdx.x * kKinWaves + wave) * a.nq) + lane) * kKinCand;
            cd[0] = candK;
            cd[1] = candS;
            cd[2] = candT;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kKinBlock) void mcalf_kin_sums_kernel(const KinArgs a) {
    __shared__ double sTab[2][kFoldTab];
    kin_pixel<false>(a, sTab);
}

__global__ __launch_bounds__(kKinBlock) void mcalf_kin_scan_kernel(const KinArgs a) {
    __shared__ double sTab[2][kFoldTab];
    kin_pixel<true>(a, sTab);
}

__global__ __launch_bounds__(64) void mcalf_kin_offsets_kernel(const KinArgs a) {
    const long rl = (long)blockIdx.x * 64 + threadIdx.x;
    if (rl >= (long)a.nrows * a.lay.nlines) return;
    const int nslabs = kin_nslabs(a);
    double* sumT = a.part + (size_t)rl * 2 * nslabs;
    const double* sumX = sumT + nslabs;
    double off = 0.0, m1 = 0.0;
    for (int s = 0; s < nslabs; ++s) {
        const double w = sumT[s];
        sumT[s] = off;
        off += w;
    }
    for (int w = 0; w < a.ntiles * kKinWaves; ++w) m1 += sumX[w];
    double* head = a.head + (size_t)rl * kKinHead;
    head[0] = off;                                                                 // I: S of the last pixel
    head[1] = a.wl[a.npix >> 1] + m1 / off;
    for (int q = 0; q < a.nq; ++q) head[2 + q] = a.q[q] * off;
}

__global__ __launch_bounds__(64) void mcalf_kin_finalize_kernel(const KinArgs a) {
    const long rl = (long)blockIdx.x * 64 + threadIdx.x;
    if (rl >= (long)a.nrows * a.lay.nlines) return;
    const int nslabs = kin_nslabs(a), nwaves = a.ntiles * kKinWaves;
    const double* head = a.head + (size_t)rl * kKinHead;
    const double I = head[0];
    const bool degenerate = !(fabs(I) <= 1.79769313486231570815e308) || I == 0.0;  // not finite, or nothing absorbs
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (a.mom) {
        const double* sumV = a.part + (size_t)rl * 2 * nslabs + nslabs;
        double v = 0.0;
        for (int w = 0; w < nwaves; ++w) v += sumV[w];
        double* mom = a.mom + (size_t)rl * 3;
        mom[0] = I;
        mom[1] = degenerate ? nan : head[1];
        mom[2] = degenerate ? nan : sqrt(v / I);
    }
    if (!a.lamq) return;
    for (int q = 0; q < a.nq; ++q) {
        double k = -1.0, Sk = I, tk = 0.0;
        for (int w = 0; w < nwaves; ++w) {
            const double* cd = a.cand + (((size_t)rl * nwaves + w) * a.nq + q) * kKinCand;
            const double kw = cd[0];
            if (kw >= 0.0 && (k < 0.0 || kw < k)) {
                k = kw;
                Sk = cd[1];
                tk = cd[2];
            }
        }
        const int ik = k >= 0.0 ? (int)k : a.npix - 1;
        double frac = 0.0;
        if (tk > 0.0) {
            frac = (Sk - head[2 + q]) / tk;
            frac = frac >= 0.0 ? (frac <= 1.0 ? frac : 1.0) : 0.0;                 // (a NaN ends at 0; the row is degenerate then)
        }
        const double e0 = a.edge[ik], e1 = a.edge[ik + 1];
        a.lamq[(size_t)rl * a.nq + q] = degenerate ? nan : e1 - (e1 - e0) * frac;
    }
}

namespace mcalf {
const void* kin_kernel_ptr(KinKernel k) {
    static const void* const table[] = {(const void*)&mcalf_kin_sums_kernel, (const void*)&mcalf_kin_offsets_kernel,
                                        (const void*)&mcalf_kin_scan_kernel, (const void*)&mcalf_kin_finalize_kernel};   // in the order of enum KinKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kKinKernelCount, "one entry per KinKernel");
    return table[k];
}
}  // namespace mcalf
