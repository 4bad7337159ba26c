// The optical depth of a fast-path (component, line) record from its y-folded table, for the analysis kernels that walk a
// spectrum tile by tile with the table in LDS: the equivalent widths (eqw_kernels.hip) and the optical-depth kinematics
// (kin_kernels.hip).  Stated once, so that both evaluate tau with the same operations in the same order.
//
//   fold_load    a thread's two entries of the universal table T[VT_NY][VT_NTOT], kept in registers for the whole kernel
//   fold_store   the record's coefficients c[idx] = scale sum_n y^n T[n][idx] into an LDS table (two per thread)
//   tau_fast     K H(u, y) of one pixel from that table
//
// Device code on top of voigt_device.h's fold_coef and fast_rcp.  Every product-and-sum in here is an explicit fma: it does not
// matter whether the including file has switched contraction to FMA off.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <hip/hip_runtime.h>

#include "theta_row.h"
#include "voigt_device.h"

namespace mcalf {

static_assert(kFastMaxA == kYFastMax, "record_kind's fast path is the folded tables' range of a");
constexpr int kFoldTab = (VT_NTOT + 7) & ~7;      // doubles per folded table in LDS

// The two table entries of thread t of a workgroup of kBlock threads: t and t + kBlock (the second only where it exists).
template <int kBlock>
__device__ __forceinline__ void fold_load(const double* __restrict__ tabs, int t, double (&T0)[VT_NY], double (&T1)[VT_NY]) {
    static_assert(2 * kBlock >= VT_NTOT, "two coefficients per thread cover the table");
    static_assert(kBlock <= VT_NCORE, "a thread's first coefficient is a core coefficient");
    const bool has1 = t + kBlock < VT_NTOT;
#pragma unroll
    for (int n = 0; n < VT_NY; ++n) {
        T0[n] = tabs[n * VT_NTOT + t];
        T1[n] = has1 ? tabs[n * VT_NTOT + t + kBlock] : 0.0;
    }
}

// The thread's two coefficients of a record (a = y, scale K; the wing zones carry K y / sqrt(pi)) into `tab`.  The caller
// puts a barrier between this and the first tau_fast on `tab`.
template <int kBlock>
__device__ __forceinline__ void fold_store(double* __restrict__ tab, const double (&T0)[VT_NY], const double (&T1)[VT_NY], int t, double y,
                                           double K, double Kyt) {
    const int i1 = t + kBlock;
    tab[t] = fold_coef(T0, y, K);
    if (i1 < VT_NTOT) tab[i1] = fold_coef(T1, y, i1 < VT_NCORE ? K : Kyt);
}

// K H(u, y) of a fast-path line from its folded table: what a directly evaluated pixel of the fused kernel gets
// (kernels.hip: eval_line) -- the core table for every |u| < 8, the two wing zones in 1/u^2 beyond.
__device__ __forceinline__ double tau_fast(const double* __restrict__ tab, double u) {
    const double x2 = u * u;
    double t, P;
    if (x2 >= kX2Far) {
        t = fast_rcp(x2);
        const double* c = tab + VT_ZF_OFF;
        P = c[VT_FDEG];
#pragma unroll
        for (int k = VT_FDEG - 1; k >= 0; --k) P = fma(P, t, c[k]);
    } else if (x2 >= kX2Wing) {
        t = fast_rcp(x2);
        const double* c = tab + VT_Z0_OFF;
        P = c[VT_WDEG];
#pragma unroll
        for (int k = VT_WDEG - 1; k >= 0; --k) P = fma(P, t, c[k]);
    } else {                                                  // |u| < 8, or NaN (interval 0, the result is NaN)
        const double x4 = fabs(u) * 4.0;
        const int jx = min(max((int)x4, 0), VT_NINT - 1);
        const double s = fma(x4, 2.0, -(double)(2 * jx + 1));
        const double* c = tab + jx * VT_CSTRIDE;
        P = c[VT_CDEG];
#pragma unroll
        for (int k = VT_CDEG - 1; k >= 0; --k) P = fma(P, s, c[k]);
        t = 1.0;
    }
    return t * P;
}

}  // namespace mcalf
