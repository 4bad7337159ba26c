// How a parameter row (theta) is read -- the rules of the reference fitter's reconstruct_spec (hires_fitter.py:409-449, JAX
// path :571-616), each stated ONCE for every kernel family outside the fused translation unit: the derivative kernels
// (grad_kernels.hip), the equivalent widths (eqw_kernels.hip) and the fit (fit_kernels.hip), with their host sides.
//
//     [R] [cont] ncomp (N, z, b) x ncompmax (N, z, b) x nfill          R / cont only where they are free
//                ^startind                  ^endind                      (ctx_plan.h: plan_shape sets the three indices)
//
// Plain C++ that compiles for the host and for the device from one source (no HIP intrinsics, no libm call but floor / trunc /
// ceil / fabs), so tests/stubs/theta_row_check.cpp runs every rule on the CPU (tests/test_theta_row_host.py).
//
// The fused translation unit (kernels.hip with sample_setup.h and wide_lsf.h) keeps its OWN text of these rules: its code
// object is the one every headline number hangs on, and a call to an identical inline function reorders a third of its
// machine code.  tests/test_gpu_theta_row.py ties that copy to this header by behaviour: the fused kernel must treat a row
// exactly as the count, the columns and the skipped slots defined here say.
#pragma once
#include <cmath>

#include "kernel_args.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCALF_ROW_FN __host__ __device__ __forceinline__
#else
#define MCALF_ROW_FN inline
#endif

namespace mcalf {

// The layout of a context's rows and what stands in for the columns it does not have.  jax: the JAX path's semantics
// (conv_mode MCALF_CONV_SAME_EDGE_JAX) -- floor on the count slot, the fixed LSF grid.
struct RowLayout {
    int ndim, nlines, ncompmax, nfill, startind, endind, freespecres, freecont, jax;
    double specres_fixed, contval_fixed;
};

// Active components from the value of the count slot p[startind]: int() on the numpy path (:428, truncation), floor on the JAX
// path (:616), clamped to [0, ncompmax].  The two differ on (-1, 0) alone, where both end at 0.  NaN and -inf give 0 (no
// comparison with NaN holds), +inf and everything from ncompmax up give ncompmax; the double is only converted to int inside
// [1, ncompmax).
MCALF_ROW_FN int active_components(const RowLayout& lay, double count_slot_value) {
    const double nct = lay.jax ? std::floor(count_slot_value) : std::trunc(count_slot_value);
    return (nct >= 1.0) ? ((nct >= (double)lay.ncompmax) ? lay.ncompmax : (int)nct) : 0;
}

// First of the three columns (N, z, b) of target component c (:431) and of filler k (:439); the continuum's column.
MCALF_ROW_FN int target_col(const RowLayout& lay, int c) { return 1 + 3 * c + lay.startind; }
MCALF_ROW_FN int filler_col(const RowLayout& lay, int k) { return 3 * k + lay.endind; }
MCALF_ROW_FN int cont_col(const RowLayout& lay) { return lay.freespecres ? 1 : 0; }

// R and the continuum of row p (:412-425 / :571-572).
MCALF_ROW_FN double row_resolution(const RowLayout& lay, const double* p) { return lay.freespecres ? p[0] : lay.specres_fixed; }
MCALF_ROW_FN double row_continuum(const RowLayout& lay, const double* p) { return lay.freecont ? p[cont_col(lay)] : lay.contval_fixed; }

// Whether coordinate k of a row with nc active components means anything continuous: not the count slot, not the (N, z, b) of
// a slot at or beyond the count (the likelihood never reads those, the fit never moves them).
MCALF_ROW_FN bool coord_movable(const RowLayout& lay, int nc, int k) {
    if (k == lay.startind) return false;
    const int rel = k - target_col(lay, 0);
    return !(rel >= 3 * nc && rel < 3 * lay.ncompmax);
}

// A (component, line) record: u = nu A - B, a the damping parameter, tau = K H(u, a).  ONE division, 1/dnu = wrest / b (:360
// with :376's b * 1e5); what the reference divides by dnu is multiplied by it (:361-365).  Products only: nothing to contract.
// cold = 10^logN (:357) is the caller's: the fused path forms it with its own pow10_fast, the kernels here with pow().
struct LineScale { double rdnu, zp1, A, B, a, K; };

MCALF_ROW_FN LineScale line_scale(double z, double b, const LineDev& ln, double cold) {
    LineScale s;
    s.zp1 = z + 1.0;                                     // :358
    s.rdnu = ln.wrest_cm / (b * 1e5);
    s.A = s.zp1 * s.rdnu;                                // :362
    s.B = ln.nujk * s.rdnu;
    s.a = ln.gamma4pi * s.rdnu;                          // :361
    s.K = kTauConst * cold * ln.f * s.rdnu;              // :364-365
    return s;
}

// How a record is evaluated.  Fast: the y-folded tables, a in [0, kFastMaxA] (voigt_device.h: kYFastMax).  General: any other
// a (NaN too), and columns so absurd that exp(-x^2) matters past |x| = 8.  Zero: |1 + z| beyond 1e100 with finite a and K --
// every |u| overflows, the reference's wofz returns 0 and the line adds exactly nothing; a NaN anywhere stays NaN instead.
enum RecordKind : int { kRecFast = 1, kRecGeneral = 2, kRecZero = 3 };
constexpr double kFastMaxA = 0.00390625;                 // 2^-8

MCALF_ROW_FN RecordKind record_kind(double zp1, double a, double K) {
    RecordKind kind = kRecFast;
    if (!(a <= kFastMaxA) || !(a >= 0.0)) kind = kRecGeneral;
    else if (K * 1.6e-28 > 2e-17) kind = kRecGeneral;
    if (!(std::fabs(zp1) < 1e100) && zp1 == zp1 && std::fabs(K) < 1e100 && std::fabs(a) < 1e100) kind = kRecZero;
    return kind;
}

// LSF half-width in pixels of a row of resolution R (FWHM, km/s).  numpy path: none unless R > velstep (:445; a NaN R fails
// that test as it does in the reference, and has no taps), else astropy's ceil(kKernelReach sigma) (:458); `bad` when that is
// not within the n_cap the context provisions (R = +inf included).  JAX path: the context's fixed grid (:549-560), never bad.
struct LsfWidth { int n; bool bad; };

MCALF_ROW_FN LsfWidth lsf_half_width(double R, double velstep, int jax, int jax_half, int n_cap) {
    LsfWidth w = {0, false};
    if (jax) {
        w.n = jax_half;
    } else if (R > velstep) {
        const double sigma = (R / kFwhmToSigma) / velstep;   // :454
        const double nd = std::ceil(kKernelReach * sigma);
        if (!(nd <= (double)n_cap)) w.bad = true;
        else w.n = (int)nd;
    }
    return w;
}

}  // namespace mcalf
