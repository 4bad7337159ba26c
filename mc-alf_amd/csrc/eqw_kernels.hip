// The equivalent-width kernels for gfx950, float64 (mcalf_eqw_batch): per row the rest-frame width of every (component, line)
// and the observed-frame width of every line's blended profile, without a spectrum ever reaching memory.
//
//     Wcomp[c, l]  = ( sum_pix (1 - exp(-tau_cl(pix))) dlam[pix] ) / (1 + z_c)         hires_fitter.py:481-489
//     Wblend[l]    =   sum_pix (1 - exp(-sum_c tau_cl(pix))) dlam[pix]
//
// tau is the likelihood's: the y-folded tables of voigt_device.h for a in [0, 2^-8], hjert_general for everything else
// (a negative "b" of the as-written indexing, absurd columns), and the record arithmetic of theta_row.h (line_scale,
// record_kind).  Nothing is convolved and the continuum does not enter (the reference's (cont v) / cont).
//
//   setup     one workgroup per row: the slots decoded under a.indexing, one record per (slot, line)
//   pixel     workgroup = (row, tile of kEqwTile pixels).  Lines outer, slots inner, so the blend needs ONE running sum
//             of tau per pixel whatever nlines is.  Per (slot, line) the workgroup folds the line's coefficients into LDS
//             once (two per thread, the thread's table entries stay in registers for the whole kernel; the two LDS
//             tables alternate, so a record costs one barrier), every thread evaluates its kEqwPpt pixels from them and
//             sums its terms in pixel order; the wave's 64 sums go through a fixed butterfly and lane 0 stores the
//             wave's partial.
//   finalize  one thread per output cell: tiles in order, inside a tile the waves in order, then / (1 + z).
// No atomics and one summation order: a row's bits do not depend on its batch, its position, its pass, the outputs
// requested or the device.
#include <hip/hip_runtime.h>

#include "eqw_args.h"
#include "tau_fold.h"
#include "voigt_device.h"
#include "wave_row.h"

using namespace mcalf;

namespace {

__device__ __forceinline__ int eqw_nrec(const EqwArgs& a) { return a.lay.ncompmax * a.lay.nlines; }
__device__ __forceinline__ int eqw_ncells(const EqwArgs& a) { return (a.lay.ncompmax + 1) * a.lay.nlines; }

// sum_j (1 - exp(-tau_j)) dlam_j over the thread's valid pixels, in pixel order.
__device__ __forceinline__ double width_terms(const double (&tau)[kEqwPpt], const double (&dl)[kEqwPpt], unsigned valid) {
    double w = 0.0;
#pragma unroll
    for (int j = 0; j < kEqwPpt; ++j) w += ((valid >> j) & 1u) ? (1.0 - exp_neg(tau[j])) * dl[j] : 0.0;
    return w;
}

}  // namespace

__global__ __launch_bounds__(64) void mcalf_eqw_setup_kernel(const EqwArgs a) {
    const int r = blockIdx.x;
    const double* p = a.P + (size_t)r * a.lay.ndim;
    const bool layout = a.indexing == kEqwIndexLayout;
    const int nc = layout ? active_components(a.lay, p[a.lay.startind]) : a.lay.ncompmax;   // as written: every slot (:481)
    const int nrec = eqw_nrec(a);
    for (int k = threadIdx.x; k < nrec; k += 64) {
        const int c = k / a.lay.nlines;
        double* rec = a.recs + ((size_t)r * nrec + k) * kEqwRec;
        if (c >= nc) {                                                             // its parameters are never read
#pragma unroll
            for (int i = 0; i < kEqwRec; ++i) rec[i] = 0.0;                        // (kind = kEqwInactive)
            continue;
        }
        const LineDev ln = a.lines[k - c * a.lay.nlines];
        const int q = target_col(a.lay, c) - (layout ? 0 : 1);                     // as written: one column early (:482)
        const double logN = p[q], z = p[q + 1], b = p[q + 2];
        const LineScale s = line_scale(z, b, ln, pow(10.0, logN));
        rec[0] = s.A;                                                              // u = nu A - B
        rec[1] = s.B;
        rec[2] = s.a;
        rec[3] = s.K;
        rec[4] = s.K * s.a * kInvSqrtPi;
        rec[5] = (double)record_kind(s.zp1, s.a, s.K);
        rec[6] = s.zp1;
        rec[7] = 0.0;
    }
}

__global__ __launch_bounds__(kEqwBlock) void mcalf_eqw_pixel_kernel(const EqwArgs a) {
    __shared__ double sTab[2][kFoldTab];
    const int r = blockIdx.y, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    double T0[VT_NY], T1[VT_NY];                                                   // the thread's two coefficients of every fold: table entries t and t + kEqwBlock
    fold_load<kEqwBlock>(a.tabs, t, T0, T1);
    double nu[kEqwPpt], dl[kEqwPpt];
    unsigned valid = 0;
#pragma unroll
    for (int j = 0; j < kEqwPpt; ++j) {
        const int i = blockIdx.x * kEqwTile + j * kEqwBlock + t;
        const bool ok = i < a.npix;
        nu[j] = a.nu[ok ? i : a.npix - 1];
        dl[j] = ok ? a.dlam[i] : 0.0;
        valid |= ok ? (1u << j) : 0u;
    }
    const int nrec = eqw_nrec(a);
    const double* recs = a.recs + (size_t)r * nrec * kEqwRec;
    double* part = a.part + ((size_t)r * a.ntiles + blockIdx.x) * eqw_ncells(a) * kEqwWaves;
    const bool wantComp = a.Wcomp != nullptr, wantBlend = a.Wblend != nullptr;
    int buf = 0;
    for (int l = 0; l < a.lay.nlines; ++l) {
        double st[kEqwPpt];                                                        // running sum of tau over the slots, per pixel
#pragma unroll
        for (int j = 0; j < kEqwPpt; ++j) st[j] = 0.0;
        for (int c = 0; c < a.lay.ncompmax; ++c) {
            const int cell = c * a.lay.nlines + l;
            const double* rec = recs + (size_t)cell * kEqwRec;
            const int kind = __builtin_amdgcn_readfirstlane((int)rec[5]);          // the same for the whole workgroup: a scalar branch
            if (kind != (int)kEqwFast && kind != (int)kEqwGeneral) continue;
            const double A = rec[0], B = rec[1], y = rec[2], K = rec[3];
            double tau[kEqwPpt];
            if (kind == (int)kEqwFast) {
                const double Kyt = rec[4];
                double* tab = sTab[buf];
                fold_store<kEqwBlock>(tab, T0, T1, t, y, K, Kyt);
                __syncthreads();                                                   // (the other table is still being read by slower waves)
                buf ^= 1;
#pragma unroll
                for (int j = 0; j < kEqwPpt; ++j) tau[j] = tau_fast(tab, fma(nu[j], A, -B));
            } else {
#pragma unroll
                for (int j = 0; j < kEqwPpt; ++j) tau[j] = K * hjert_general(fabs(fma(nu[j], A, -B)), y);
            }
            if (wantBlend) {
#pragma unroll
                for (int j = 0; j < kEqwPpt; ++j) st[j] += tau[j];
            }
            if (wantComp) {
                const double w = wave_sum(width_terms(tau, dl, valid));
                if (lane == 0) part[cell * kEqwWaves + wave] = w;
            }
        }
        if (wantBlend) {
            const double w = wave_sum(width_terms(st, dl, valid));
            if (lane == 0) part[(nrec + l) * kEqwWaves + wave] = w;
        }
    }
}

__global__ __launch_bounds__(256) void mcalf_eqw_finalize_kernel(const EqwArgs a) {
    const int nrec = eqw_nrec(a), ncells = eqw_ncells(a);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.nrows * ncells) return;
    const int r = (int)(idx / ncells), cell = (int)(idx - (long)r * ncells);
    const bool comp = cell < nrec;
    if (comp ? !a.Wcomp : !a.Wblend) return;
    double kind = kEqwFast, zp1 = 1.0;
    if (comp) {
        const double* rec = a.recs + ((size_t)r * nrec + cell) * kEqwRec;
        kind = rec[5];
        zp1 = rec[6];
    }
    double s = 0.0;
    if (kind == kEqwFast || kind == kEqwGeneral) {                                 // (the pixel kernel wrote nothing for the others)
        for (int tile = 0; tile < a.ntiles; ++tile) {
            const double* w = a.part + (((size_t)r * a.ntiles + tile) * ncells + cell) * kEqwWaves;
#pragma unroll
            for (int k = 0; k < kEqwWaves; ++k) s += w[k];
        }
    }
    if (!comp) a.Wblend[(size_t)r * a.lay.nlines + (cell - nrec)] = s;
    else a.Wcomp[(size_t)r * nrec + cell] = (kind == kEqwInactive) ? 0.0 : s / zp1;    // :489
}

namespace mcalf {
const void* eqw_kernel_ptr(EqwKernel k) {
    static const void* const table[] = {(const void*)&mcalf_eqw_setup_kernel, (const void*)&mcalf_eqw_pixel_kernel,
                                        (const void*)&mcalf_eqw_finalize_kernel};   // in the order of enum EqwKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kEqwKernelCount, "one entry per EqwKernel");
    return table[k];
}
}  // namespace mcalf
