// Device Faddeeva function w(z) and its derivative w'(z) for the gradient path (grad_kernels.hip), float64, Im z >= 0.
//
// H(x, y) = Re w(x + i y) is the Voigt-Hjerting function the likelihood uses; the gradient needs its partials too:
//     w'(z) = -2 z w(z) + 2 i / sqrt(pi),   H_x = Re w',   H_y = -Im w'.
// The fused kernel's folded tables (voigt_device.h) are built for H alone; this file evaluates w directly:
//
//   |z| <   8 : Weideman's rational expansion (SIAM J. Numer. Anal. 31 (1994) 1497) with N = 40 terms,
//               w = 2 p(Z) / (L - i z)^2 + (1/sqrt(pi)) / (L - i z),   Z = (L + i z) / (L - i z),   L = sqrt(N / sqrt 2);
//               w' from the identity above (cancellation grows like 2|z|^2: <= 2e-13 relative at |z| = 8)
//   |z| >=  8 : the Laplace asymptotic series  w = i/(sqrt(pi) z) sum_k (2k-1)!!/(2 z^2)^k, truncated by |z| (asym_terms:
//               24 terms at |z| = 8 down to 4 from |z| = 1000, the bulk of a spectrum's pixels),
//               its term-by-term derivative and that of z w (no cancellation)
//
// Accuracy, measured ON THE DEVICE against 120-digit mpmath (tests/test_gpu_voigt_grad.py; the 3871 points of
// tests/golden/voigt_grad_reference.npz: y in {0, 1e-9 ... 30}, |x| <= 1e8, both sides of |z| = 8 and of every bracket of
// asym_terms), worst case per region:
//   |z| <  8 : |dw| <= 1.0e-15 |w|, |dw'| <= 6.0e-14 |w'| (complex; claimed: 5e-15, 2e-13); e, and the d2, e2, e3 of
//              faddeeva_d2w, within 5.0 eps M_q, eps = 2^-53, M_q the magnitudes that the identity of q adds up
//              (M_w' = 2|z||w| + 2/sqrt(pi), M_e = |w| + |z| M_w', ...).  As a fraction of the VALUE that is much more just
//              inside |z| = 8 at small y: at y = 1e-4, 6 <= |x| < 8, e 4.0e-8, d2 4.0e-8, e2 1.1e-6, e3 3.9e-6
//              (DESIGN section 3.8 has the table)
//   |z| >= 8 : every output within 8.8e-16 of the magnitude of its complex quantity; as a fraction of the value itself
//              wr, wi, dr, di, e2 <= 1.6e-15, and e 2.0e-15, d2 4.0e-15, e3 4.4e-15, worst next to the zeros of their real
//              parts (Re (z w)' and Re w'' vanish on x = y/sqrt 3; asym_lead below).  exp(-x^2) <= 1.6e-28 is dropped, so
//              at y = 0 the real parts are 0.
// The 40 coefficients are Weideman's FFT of exp(-t^2)(L^2 + t^2) on t = L tan(theta/2), highest degree first (his `cef`
// routine, evaluated in float64).
#pragma once
#include <hip/hip_runtime.h>

namespace mcalf {

constexpr double kWeidL = 5.3182958969449885;
constexpr int kWeidN = 40;
constexpr double kGradInvSqrtPi = 0.56418958354775628695;
constexpr double kAsymR2 = 64.0;      // |z|^2 from which the asymptotic series takes over

// Terms of the asymptotic series that keep w, w' and (z w)' within about 1e-15 relative over [|z|, next threshold) (on the device
// against 120-digit mpmath at both edges of every bracket, see above; the truncation error falls as |z| grows inside each
// bracket).  (z w)' starts at the k = 1 term, so its
// relative truncation error is 2k|z|^2 times the last term's: that, not w, sets the counts.
__device__ __forceinline__ int asym_terms(double r2) {
    return r2 >= 1e6 ? 4 : r2 >= 1e4 ? 6 : r2 >= 900.0 ? 9 : r2 >= 225.0 ? 14 : 24;
}

__device__ __constant__ static const double kWeidCoef[kWeidN] = {
    -1.73569809987918647e-15, 1.20167491075928095e-15, 1.15191702207494847e-14, -5.23171636632440398e-15,
    -7.07108802215940845e-14, 1.37782240476640457e-14, 4.53414489094346555e-13, 1.20333095291956798e-13,
    -2.90771851041427015e-12, -2.72777356258302445e-12, 1.77141856738671790e-11, 3.47274209389070152e-11,
    -9.05513886095832302e-11, -3.56323504036026841e-10, 2.10859907312510581e-10, 3.01778042555156406e-09,
    3.24974658294507890e-09, -1.83156168342968342e-08, -6.35177348301541098e-08, 1.41986423729534295e-08,
    5.91213695302905726e-07, 1.48356611331720142e-06, -1.06601389841627292e-06, -1.80074471447234073e-05,
    -5.59130926423487940e-05, -3.93936314548380510e-05, 4.39807015986967025e-04, 2.70540563307372899e-03,
    1.00481862427835352e-02, 2.92029164712418812e-02, 7.18236177907432827e-02, 1.55042638024795038e-01,
    2.99894379961500590e-01, 5.26652898827708604e-01, 8.47217457659381501e-01, 1.25638156757651331e+00,
    1.72538308481797786e+00, 2.20151379487831189e+00, 2.61605415276185971e+00, 2.89962450938970484e+00,
};

// Re (i / (sqrt(pi) z^3)) = y (3 x^2 - y^2) / (sqrt(pi) |z|^6), rr2 = 1/|z|^2, rm2 = 1/|z|^4: the leading term of the series of
// (z w)' (times -1), of w'' (times 2) and of (z^2 w)''.  It vanishes on x = y / sqrt 3; taken as the real part of a complex
// product it keeps there only ~1e-16 of the term's MAGNITUDE, which next to the zero left those three real parts with 1e-14
// to 6e-14 of their value.  In real arithmetic, with the roundings of x^2 and y^2 put back, the difference is good to an ulp.
__device__ __forceinline__ double asym_lead(double x, double y, double rr2, double rm2) {
    const double p = y * y, pe = fma(y, y, -p), q = x * x, qe = fma(x, x, -q);
    return y * (fma(3.0, q, -p) + (3.0 * qe - pe)) * kGradInvSqrtPi * rr2 * rm2;
}

// (wr, wi) = w(x + i y), (dr, di) = w'(x + i y), e = Re(w + z w') = H + x H_x + y H_y; y >= 0.
// e is what d tau / d b needs; in the wings its terms cancel to O(1/|z|^2) of H (a damped line's Lorentzian wing does not
// depend on b), so beyond |z| = 8 it is summed from its own series, (z w)' = i/sqrt(pi) sum_k -2k c_k z^(-2k-1).
__device__ __forceinline__ void faddeeva_dw(double x, double y, double& wr, double& wi, double& dr, double& di, double& e) {
    const double r2 = x * x + y * y;
    if (r2 >= kAsymR2) {
        // 1/(2 z^2) and the two sums s = sum c_k, sd = -sum (2k+1) c_k, c_0 = 1, c_{k+1} = c_k (2k+1)/(2 z^2)
        // ONE division: 1/|z|^2, and |z^2|^2 = |z|^4
        const double z2r = x * x - y * y, z2i = 2.0 * x * y;
        const double rr2 = 1.0 / r2, rm2 = rr2 * rr2;
        const double hr = 0.5 * z2r * rm2, hi = -0.5 * z2i * rm2;
        double cr = 1.0, ci = 0.0, sr = 0.0, si = 0.0, tr = 0.0, ti = 0.0, er = 0.0, ei = 0.0;
        const int nt = asym_terms(r2);
        for (int k = 0; k < nt; ++k) {
            sr += cr; si += ci;
            tr -= (2 * k + 1) * cr; ti -= (2 * k + 1) * ci;
            if (k != 1) { er -= (2 * k) * cr; ei -= (2 * k) * ci; }     // (k = 1 is asym_lead)
            const double f = (double)(2 * k + 1);
            const double nr = f * (cr * hr - ci * hi), ni = f * (cr * hi + ci * hr);
            cr = nr; ci = ni;
        }
        // i/(sqrt(pi) z) = i conj(z) / (sqrt(pi) |z|^2) = (y + i x) / (sqrt(pi) r2)
        const double ar = y * kGradInvSqrtPi * rr2, ai = x * kGradInvSqrtPi * rr2;
        wr = ar * sr - ai * si;
        wi = ar * si + ai * sr;
        e = (ar * er - ai * ei) - asym_lead(x, y, rr2, rm2);
        // i/(sqrt(pi) z^2) = i conj(z^2) / (sqrt(pi) |z|^4)
        const double br = z2i * kGradInvSqrtPi * rm2, bi = z2r * kGradInvSqrtPi * rm2;
        dr = br * tr - bi * ti;
        di = br * ti + bi * tr;
        return;
    }
    // L - i z = (L + y) - i x,  L + i z = (L - y) + i x
    const double er = kWeidL + y, ei = -x;
    const double em = er * er + ei * ei;
    const double vr = er / em, vi = -ei / em;                     // 1/(L - i z)
    const double ur = kWeidL - y, ui = x;
    const double Zr = ur * vr - ui * vi, Zi = ur * vi + ui * vr;  // Z
    double pr = kWeidCoef[0], pi = 0.0;
#pragma unroll
    for (int k = 1; k < kWeidN; ++k) {
        const double nr = fma(pr, Zr, fma(-pi, Zi, kWeidCoef[k]));
        pi = fma(pr, Zi, pi * Zr);
        pr = nr;
    }
    const double v2r = vr * vr - vi * vi, v2i = 2.0 * vr * vi;
    wr = 2.0 * (pr * v2r - pi * v2i) + kGradInvSqrtPi * vr;
    wi = 2.0 * (pr * v2i + pi * v2r) + kGradInvSqrtPi * vi;
    // w' = -2 z w + 2 i / sqrt(pi)
    dr = -2.0 * (x * wr - y * wi);
    di = -2.0 * (x * wi + y * wr) + 2.0 * kGradInvSqrtPi;
    e = wr + (x * dr - y * di);
}

// Second order, for the Hessian-vector product of logL (mcalf_hvp_deriv_kernel).  With K H(u, a), u and a both ~ 1/b:
//     d2tau/dz2 ~ Re w'',   d2tau/dz db ~ Re (z w)'' = Re (2 w' + z w''),   d2tau/db2 ~ Re (z^2 w)'' = Re (2 (z w)' + z (z w)'')
// Outputs: wr = Re w, dr = Re w', e = Re (z w)' as faddeeva_dw gives them, d2 = Re w'', e2 = Re (z w)'', e3 = Re (z^2 w)''.
//   |z| <  8 : algebraic from w and w':  w'' = -2 (w + z w'),  then the two identities above
//   |z| >= 8 : every combination from its OWN series, differentiated term by term -- in a Lorentzian wing (z w)'' and
//              (z^2 w)'' cancel to O(|z|^-2) and O(|z|^-4) of their O(1) terms, which leaves no digit of the algebraic form:
//                  w''       = i/(sqrt(pi) z^3) sum_k (2k+1)(2k+2) c_k      (z w)''   = i/(sqrt(pi) z^2) sum_k 2k (2k+1) c_k
//                  (z^2 w)'' = i/(sqrt(pi) z)   sum_k 2k (2k-1) c_k         c_k = (2k-1)!!/(2 z^2)^k
//              two terms more than asym_terms: the second derivatives weigh the last term 2k times heavier than the first.
__device__ __forceinline__ void faddeeva_d2w(double x, double y, double& wr, double& dr, double& e, double& d2, double& e2,
                                             double& e3) {
    const double r2 = x * x + y * y;
    if (r2 >= kAsymR2) {
        const double z2r = x * x - y * y, z2i = 2.0 * x * y;
        const double rr2 = 1.0 / r2, rm2 = rr2 * rr2;
        const double hr = 0.5 * z2r * rm2, hi = -0.5 * z2i * rm2;
        double cr = 1.0, ci = 0.0, sr = 0.0, si = 0.0, tr = 0.0, ti = 0.0, er = 0.0, ei = 0.0;
        double ur = 0.0, ui = 0.0, pr = 0.0, pi = 0.0, qr = 0.0, qi = 0.0;
        const int nt = asym_terms(r2) + 2;
        for (int k = 0; k < nt; ++k) {
            const double f = (double)(2 * k + 1), g = (double)(2 * k);
            sr += cr; si += ci;
            tr -= f * cr; ti -= f * ci;
            // the term in 1/z^3 of (z w)', w'' and (z^2 w)'' is asym_lead
            if (k != 1) { er -= g * cr; ei -= g * ci; }
            if (k != 0) { ur += f * (g + 2.0) * cr; ui += f * (g + 2.0) * ci; }      // w''
            pr += g * f * cr; pi += g * f * ci;                                      // (z w)''
            if (k != 1) { qr += g * (g - 1.0) * cr; qi += g * (g - 1.0) * ci; }      // (z^2 w)''
            const double nr = f * (cr * hr - ci * hi), ni = f * (cr * hi + ci * hr);
            cr = nr; ci = ni;
        }
        // i/(sqrt(pi) z), i/(sqrt(pi) z^2) as in faddeeva_dw; i/(sqrt(pi) z^3) = (i/(sqrt(pi) z^2)) conj(z) / |z|^2
        const double ar = y * kGradInvSqrtPi * rr2, ai = x * kGradInvSqrtPi * rr2;
        const double br = z2i * kGradInvSqrtPi * rm2, bi = z2r * kGradInvSqrtPi * rm2;
        const double gr = (br * x + bi * y) * rr2, gi = (bi * x - br * y) * rr2;
        const double lead = asym_lead(x, y, rr2, rm2);
        wr = ar * sr - ai * si;
        e = (ar * er - ai * ei) - lead;
        e3 = (ar * qr - ai * qi) + lead;
        dr = br * tr - bi * ti;
        e2 = br * pr - bi * pi;
        d2 = (gr * ur - gi * ui) + 2.0 * lead;
        return;
    }
    double wi, di;
    faddeeva_dw(x, y, wr, wi, dr, di, e);
    const double Ei = wi + (x * di + y * dr);                      // Im (z w)'
    const double d2i = -2.0 * Ei;
    d2 = -2.0 * e;                                                 // w'' = -2 (z w)'
    const double e2i = 2.0 * di + (x * d2i + y * d2);
    e2 = 2.0 * dr + (x * d2 - y * d2i);                            // (z w)'' = 2 w' + z w''
    e3 = 2.0 * e + (x * e2 - y * e2i);                             // (z^2 w)'' = 2 (z w)' + z (z w)''
}

}  // namespace mcalf
