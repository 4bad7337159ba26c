// The analytic gradient of logL (mcalf_loglike_grad_batch, host_grad.cpp) for gfx950, float64.
//
// With w = 1/err^2, m = cont L(F), F = exp(-sum tau) and q_i = w_i (d_i - m_i) (0 on the pixels nansum drops):
//     dlogL/dtheta = sum_i q_i dm_i/dtheta
//     cont : sum_i q_i L(F)_i                 R : sum_i q_i cont (dL/dR)(F)_i      (dw_k/dsigma = w_k (k^2 - sum_j w_j j^2) / sigma^3)
//     N, z, b of a component : sum_i g_i dtau_i/dtheta,   g = -F cont L^T q
// L is the context's convolution: the periodic one with the astropy tap count on the numpy path (none when R <= velstep),
// the fixed grid with the edge reset on the JAX path; L^T is its transpose.  Per (component, line), K = cne/dnu:
//     dtau/dN = ln10 tau,   dtau/dz = K H_u (c/lambda)/dnu,   dtau/db = -(K/b)(H + u H_u + a H_a)
//
// Six kernels per pass over a block of rows, every reduction in a fixed order (no atomics): a row's bits do not depend
// on its batch, its pass or its device.
//   setup    one workgroup per row: decode, (component, line) records, normalised taps and their R derivative
//   forward  (tile, row): F = exp(-tau)                                  -> F workspace
//   model    (tile, row): m = cont L(F), q; continuum and R partials     -> q workspace, partials
//   adjoint  (tile, row): g = -F cont (L^T q)_i                          -> F workspace (in place)
//   deriv    (tile, row): H, H_u, H_a of every active (component, line); per component the three weighted sums
//   finalize (row, column): partials summed over tiles in order; -inf / NaN logL rows get NaN
// The convolutions read the workspace in HBM, so any LSF width the likelihood accepts works.
//
// The same file holds the model Jacobian's two products with a vector (mcalf_model_jvp_batch / _vjp_batch), J = dm/dtheta:
//   J v   (JVP)  setup, then
//     jvp_forward (tile, row): ONE Voigt pass: tau and dtau = sum_c (ln10 tau_c v_N + K H_u (nu/dnu) v_z - (K/b) e v_b),
//                              F = exp(-tau) -> F workspace, T = -F dtau -> q workspace
//     jvp_model   (tile, row): dM = cont L(T) + v_cont L(F) + v_R cont (dL/dR)(F), one tap loop over F and T
//   J^T q (VJP)  the gradient's own pass with the caller's cotangent in place of w (d - m): setup, forward, vjp_model (the
//                continuum and R partials; the q workspace pointer IS the caller's Q), adjoint, deriv, vjp_finalize (no
//                logL, so no veto rule: only rows whose tap count exceeds the cap are NaN)
// and the product of logL's exact Hessian with a vector (mcalf_loglike_hvp_batch): see the hvp kernels below.
#include <hip/hip_runtime.h>

#include "grad_args.h"
#include "voigt_grad.h"

using namespace mcalf;

namespace {

constexpr double kLn10 = 2.302585092994045684;

struct RowInfo { double R, cont; int n, nc; bool bad; double bot; };

__device__ __forceinline__ RowInfo row_info(const GradArgs& a, int r) {
    const double* w = a.rows + (size_t)r * kGradRow;
    RowInfo o;
    o.R = w[0]; o.cont = w[1]; o.n = (int)w[2]; o.nc = (int)w[3]; o.bad = w[4] != 0.0; o.bot = w[5];
    return o;
}

// Sum of v over the workgroup (kGradBlock threads), the same tree every time; every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = kGradBlock / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// Three sums at once (lds: 3 * kGradBlock doubles); the result is valid in thread 0.
__device__ __forceinline__ void block_sum3(double& x, double& y, double& z, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = x; lds[kGradBlock + t] = y; lds[2 * kGradBlock + t] = z;
    __syncthreads();
#pragma unroll
    for (int s = kGradBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
            lds[t] += lds[t + s];
            lds[kGradBlock + t] += lds[kGradBlock + t + s];
            lds[2 * kGradBlock + t] += lds[2 * kGradBlock + t + s];
        }
        __syncthreads();
    }
    x = lds[0]; y = lds[kGradBlock]; z = lds[2 * kGradBlock];
}

// Component slots of the record list: the ncompmax * nlines target slots, then the nfill filler slots.
__device__ __forceinline__ const double* rec_of(const GradArgs& a, int r, int slot) {
    return a.recs + ((size_t)r * a.nslots + slot) * kGradRec;
}

}  // namespace

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_setup_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    const int r = blockIdx.x;
    const int t = threadIdx.x;
    const double* p = a.P + (size_t)r * a.ndim;
    const double R = a.freespecres ? p[0] : a.specres_fixed;                      // hires_fitter.py:412-417 / :572
    const double cont = a.freecont ? p[a.freespecres ? 1 : 0] : a.contval_fixed;  // :419-425 / :571
    const double ncv = p[a.startind];
    const double nct = a.jax ? floor(ncv) : trunc(ncv);                          // :428 int() / :616 floor
    const int nc = (nct >= 1.0) ? ((nct >= (double)a.ncompmax) ? a.ncompmax : (int)nct) : 0;

    for (int slot = t; slot < a.nslots; slot += kGradBlock) {
        int q;
        const LineDev* ln;
        if (slot < a.ncompmax * a.nlines) {
            const int c = slot / a.nlines;
            q = 1 + 3 * c + a.startind;                                            // :431 (N, z, b)
            ln = a.lines + (slot - c * a.nlines);
        } else {
            q = 3 * (slot - a.ncompmax * a.nlines) + a.endind;                     // :439
            ln = a.lines + a.nlines;
        }
        const double logN = p[q], z = p[q + 1], b = p[q + 2];
        const double rdnu = ln->wrest_cm / (b * 1e5);                              // 1/dnu (:360, :376)
        double* rec = a.recs + ((size_t)r * a.nslots + slot) * kGradRec;
        rec[0] = (z + 1.0) * rdnu;                                                 // u = nu A - B  (:362)
        rec[1] = ln->nujk * rdnu;
        rec[2] = ln->gamma4pi * rdnu;                                              // a (:361)
        rec[3] = kTauConst * pow(10.0, logN) * ln->f * rdnu;                       // K = cne / dnu (:364-365)
        rec[4] = rdnu;
        rec[5] = 1.0 / b;
    }

    // taps: the numpy path's astropy count (none when R <= velstep), the JAX path's fixed grid
    const double sigma = (R / kFwhmToSigma) / a.velstep;
    int n = 0;
    bool bad = false;
    if (a.jax) {
        n = a.jax_half;
    } else if (R > a.velstep) {
        const double nd = ceil(kKernelReach * sigma);                               // :458
        if (!(nd <= (double)a.n_cap)) bad = true;
        else n = (int)nd;
    }
    double* taps = a.taps + (size_t)r * a.tapcap;
    double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    const double inv2s2 = 0.5 / (sigma * sigma);
    double s = 0.0;
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        s += exp(-(dk * dk) * inv2s2);
    }
    const double wsum = block_sum(s, lds);
    double m2 = 0.0;
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        const double w = (!a.jax && n == 0) ? 1.0 : exp(-(dk * dk) * inv2s2) / wsum;
        taps[k] = w;
        m2 += w * dk * dk;
    }
    m2 = block_sum(m2, lds);
    double bs = 0.0;
    const double dsig = 1.0 / (kFwhmToSigma * a.velstep * sigma * sigma * sigma);     // dsigma/dR / sigma^3
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        const double w = taps[k];
        dtaps[k] = (!a.jax && n == 0) ? 0.0 : w * (dk * dk - m2) * dsig;
        bs += w;
    }
    const double bot = block_sum(bs, lds);                                         // astropy divides by the tap sum (1 to rounding)
    if (t == 0) {
        double* w = a.rows + (size_t)r * kGradRow;
        w[0] = R; w[1] = cont; w[2] = (double)n; w[3] = (double)nc; w[4] = bad ? 1.0 : 0.0; w[5] = a.jax ? 1.0 : bot;
        w[6] = w[7] = 0.0;
    }
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_forward_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const double nu = a.nu[i];
    double tau = 0.0;
    const int nt = ri.nc * a.nlines;
    for (int slot = 0; slot < nt + a.nfill; ++slot) {
        const double* rec = rec_of(a, r, slot < nt ? slot : a.ncompmax * a.nlines + (slot - nt));
        double wr, wi, dr, di, e;
        faddeeva_dw(nu * rec[0] - rec[1], rec[2], wr, wi, dr, di, e);
        tau += rec[3] * wr;
    }
    a.F[(size_t)r * a.npix + i] = exp(-tau);
}

// kCot: q is the caller's cotangent (a.q points at it) instead of w (d - m).
template <bool kCot>
__device__ __forceinline__ void model_tile(const GradArgs& a, double* lds) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const double* F = a.F + (size_t)r * a.npix;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    const double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    double pc = 0.0, pR = 0.0;
    if (i < a.npix) {
        double conv, dconv = 0.0;
        if (a.jax) {
            const int h = ri.n;
            if (i < h || i >= a.npix - h) {
                conv = F[i];                                                       // :677-681 edge reset
            } else {
                double c = 0.0, d = 0.0;
                for (int k = 0; k <= 2 * h; ++k) {
                    const double f = F[i + k - h];
                    c += taps[k] * f;
                    d += dtaps[k] * f;
                }
                conv = c; dconv = d;
            }
        } else if (ri.n > 0) {
            const int n = ri.n;
            int j = (int)(((long)i - n) % a.npix);
            if (j < 0) j += a.npix;
            double c = 0.0, d = 0.0;
            for (int k = 0; k <= 2 * n; ++k) {                                     // periodic boundary (:463-464)
                const double f = F[j];
                c += taps[k] * f;
                d += dtaps[k] * f;
                if (++j == a.npix) j = 0;
            }
            conv = c / ri.bot; dconv = d / ri.bot;
        } else {
            conv = F[i];                                                           // R <= velstep: no convolution (:445)
        }
        double qv;
        if (kCot) {
            qv = a.q[(size_t)r * a.npix + i];
        } else {
            const double is2 = a.ispec2[i];
            const double res = a.obj[i] - ri.cont * conv;
            const double term = is2 * res * res - a.lgis[i];
            qv = isnan(term) ? 0.0 : is2 * res;                                    // the pixels nansum keeps (:294)
            a.q[(size_t)r * a.npix + i] = qv;
        }
        pc = qv * conv;
        pR = qv * ri.cont * dconv;
    }
    pc = block_sum(pc, lds);
    pR = block_sum(pR, lds);
    if (threadIdx.x == 0) {
        double* out = a.part + ((size_t)r * a.ntiles + blockIdx.x) * a.ndim;
        if (a.freespecres) out[0] = pR;
        if (a.freecont) out[a.freespecres ? 1 : 0] = pc;
        out[a.startind] = 0.0;                                                     // the ncomp slot
    }
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_model_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    model_tile<false>(a, lds);
}

__global__ __launch_bounds__(kGradBlock) void mcalf_vjp_model_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    model_tile<true>(a, lds);
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_adjoint_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const double* q = a.q + (size_t)r * a.npix;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    double rt;
    if (a.jax) {
        const int h = ri.n;
        rt = (i < h || i >= a.npix - h) ? q[i] : 0.0;
        // interior outputs o = i - k + h with tap k read pixel i
        const int klo = max(0, i + 2 * h - a.npix + 1), khi = min(2 * h, i);
        for (int k = klo; k <= khi; ++k) rt += taps[k] * q[i - k + h];
    } else if (ri.n > 0) {
        const int n = ri.n;
        int j = (int)(((long)i + n) % a.npix);
        double c = 0.0;
        for (int k = 0; k <= 2 * n; ++k) {                                         // output j read pixel i through tap k
            c += taps[k] * q[j];
            if (--j < 0) j = a.npix - 1;
        }
        rt = c / ri.bot;
    } else {
        rt = q[i];
    }
    double* F = a.F + (size_t)r * a.npix;
    F[i] = -F[i] * ri.cont * rt;
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_deriv_kernel(const GradArgs a) {
    __shared__ double lds[3 * kGradBlock];
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const bool valid = i < a.npix;
    const double g = valid ? a.F[(size_t)r * a.npix + i] : 0.0;
    const double nu = valid ? a.nu[i] : a.nu[0];
    double* out = a.part + ((size_t)r * a.ntiles + blockIdx.x) * a.ndim;
    const int ncomp = ri.nc + a.nfill;                 // active targets, then the fillers
    for (int c = 0; c < ncomp; ++c) {
        const bool fill = c >= ri.nc;
        const int slot0 = fill ? a.ncompmax * a.nlines + (c - ri.nc) : c * a.nlines;
        const int nl = fill ? 1 : a.nlines;
        double sN = 0.0, sz = 0.0, sb = 0.0;
        for (int l = 0; l < nl; ++l) {
            const double* rec = rec_of(a, r, slot0 + l);
            const double u = nu * rec[0] - rec[1], y = rec[2], K = rec[3];
            double wr, wi, dr, di, e;
            faddeeva_dw(u, y, wr, wi, dr, di, e);
            sN += K * wr;                                   // tau
            sz += K * dr * (nu * rec[4]);                   // K H_u du/dz
            sb -= K * rec[5] * e;                           // (K/b)(H + u H_u + a H_a)
        }
        sN *= g * kLn10; sz *= g; sb *= g;
        block_sum3(sN, sz, sb, lds);
        if (threadIdx.x == 0) {
            const int col = fill ? a.endind + 3 * (c - ri.nc) : 1 + 3 * c + a.startind;
            out[col] = sN; out[col + 1] = sz; out[col + 2] = sb;
        }
    }
    if (threadIdx.x == 0)
        for (int c = ri.nc; c < a.ncompmax; ++c) {     // inactive components: exactly 0
            const int col = 1 + 3 * c + a.startind;
            out[col] = out[col + 1] = out[col + 2] = 0.0;
        }
}

// kVeto: rows whose logL is -inf (veto) or NaN get NaN too (the VJP has no logL).
template <bool kVeto>
__device__ __forceinline__ void finalize_cell(const GradArgs& a) {
    const long e = (long)blockIdx.x * kGradBlock + threadIdx.x;
    if (e >= (long)a.nrows * a.ndim) return;
    const int r = (int)(e / a.ndim), k = (int)(e - (long)r * a.ndim);
    const double lg = kVeto ? a.logL[r] : 0.0;
    double s;
    if (a.rows[(size_t)r * kGradRow + 4] != 0.0 || !(lg > -INFINITY)) {
        s = NAN;                                                                    // too many taps, veto (-inf) or NaN row
    } else {
        s = 0.0;
        const double* p = a.part + (size_t)r * a.ntiles * a.ndim + k;
        for (int t = 0; t < a.ntiles; ++t) s += p[(size_t)t * a.ndim];
    }
    a.G[(size_t)r * a.ndim + k] = s;
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_finalize_kernel(const GradArgs a) { finalize_cell<true>(a); }

__global__ __launch_bounds__(kGradBlock) void mcalf_vjp_finalize_kernel(const GradArgs a) { finalize_cell<false>(a); }

// JVP, the one Voigt pass: per pixel tau and its directional derivative along the row's tangent.  The per-slot arithmetic
// is mcalf_grad_deriv_kernel's, contracted with v instead of reduced over pixels.  Records and tangent entries are
// row-uniform (scalar loads); the ncomp slot of v and the (N, z, b) of inactive components are never read.
__global__ __launch_bounds__(kGradBlock) void mcalf_jvp_forward_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const double* v = a.V + (size_t)r * a.ndim;
    const double nu = a.nu[i];
    double tau = 0.0, dtau = 0.0;
    const int ncomp = ri.nc + a.nfill;                 // active targets, then the fillers
    for (int c = 0; c < ncomp; ++c) {
        const bool fill = c >= ri.nc;
        const int slot0 = fill ? a.ncompmax * a.nlines + (c - ri.nc) : c * a.nlines;
        const int nl = fill ? 1 : a.nlines;
        const int col = fill ? a.endind + 3 * (c - ri.nc) : 1 + 3 * c + a.startind;
        double sN = 0.0, sz = 0.0, sb = 0.0;
        for (int l = 0; l < nl; ++l) {
            const double* rec = rec_of(a, r, slot0 + l);
            const double u = nu * rec[0] - rec[1], y = rec[2], K = rec[3];
            double wr, wi, dr, di, e;
            faddeeva_dw(u, y, wr, wi, dr, di, e);
            sN += K * wr;                                   // tau
            sz += K * dr * (nu * rec[4]);                   // K H_u du/dz
            sb -= K * rec[5] * e;                           // (K/b)(H + u H_u + a H_a)
        }
        tau += sN;
        dtau += kLn10 * sN * v[col] + sz * v[col + 1] + sb * v[col + 2];
    }
    const double F = exp(-tau);
    a.F[(size_t)r * a.npix + i] = F;
    a.q[(size_t)r * a.npix + i] = -F * dtau;
}

// JVP, the convolutions: dM = cont L(T) + v_cont L(F) + v_R cont (dL/dR)(F), the three modes of model_tile.
__global__ __launch_bounds__(kGradBlock) void mcalf_jvp_model_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    double* out = a.dM + (size_t)r * a.npix;
    if (ri.bad) {                                                                  // more taps than the context provisions
        out[i] = NAN;
        return;
    }
    const double* F = a.F + (size_t)r * a.npix;
    const double* T = a.q + (size_t)r * a.npix;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    const double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    const double* v = a.V + (size_t)r * a.ndim;
    const double vR = a.freespecres ? v[0] : 0.0;
    const double vc = a.freecont ? v[a.freespecres ? 1 : 0] : 0.0;
    double cF, cT, dF = 0.0;
    if (a.jax) {
        const int h = ri.n;
        if (i < h || i >= a.npix - h) {
            cF = F[i]; cT = T[i];                                                  // edge reset
        } else {
            double c = 0.0, d = 0.0, ct = 0.0;
            for (int k = 0; k <= 2 * h; ++k) {
                const double f = F[i + k - h];
                c += taps[k] * f;
                d += dtaps[k] * f;
                ct += taps[k] * T[i + k - h];
            }
            cF = c; dF = d; cT = ct;
        }
    } else if (ri.n > 0) {
        const int n = ri.n;
        int j = (int)(((long)i - n) % a.npix);
        if (j < 0) j += a.npix;
        double c = 0.0, d = 0.0, ct = 0.0;
        for (int k = 0; k <= 2 * n; ++k) {                                         // periodic boundary
            const double f = F[j];
            c += taps[k] * f;
            d += dtaps[k] * f;
            ct += taps[k] * T[j];
            if (++j == a.npix) j = 0;
        }
        cF = c / ri.bot; dF = d / ri.bot; cT = ct / ri.bot;
    } else {
        cF = F[i]; cT = T[i];                                                      // R <= velstep: no convolution
    }
    out[i] = ri.cont * cT + vc * cF + vR * ri.cont * dF;
}

// ---- The Hessian-vector product of logL (mcalf_loglike_hvp_batch): forward mode over the gradient's reverse pass. ----
// With d(.) the directional derivative along the row's tangent v, T = dF (jvp_forward) and dM = d m (jvp_model's sum):
//     q = W (d - m),  dq = -W dM                                          (W = 1/err^2 on the pixels nansum keeps, else 0)
//     (H v)_cont = sum_i [dq L(F) + q (L(T) + v_R (dL/dR) F)]
//     (H v)_R    = sum_i [dq cont (dL/dR) F + q v_cont (dL/dR) F + q cont ((dL/dR) T + v_R (d2L/dR2) F)]
//     g = -F cont L^T q,   dg = -T cont L^T q - F v_cont L^T q - F cont v_R (dL/dR)^T q - F cont L^T dq
//     (H v)_k    = sum_i [dg_i dtau_i/dtheta_k + g_i sum_k' d2tau_i/dtheta_k dtheta_k' v_k']      k, k' the (N, z, b) of ONE component
// Per (component, line), s = nu/dnu (du/dz), z = u + i a ~ 1/b:
//     d2tau/dN dtheta = ln10 dtau/dtheta,   d2tau/dz2 = K s^2 Re w'',   d2tau/dz db = -(K s/b) Re (z w)'',   d2tau/db2 = (K/b^2) Re (z^2 w)''
// A pass: setup, hvp_taps, jvp_forward, hvp_model, hvp_adjoint, hvp_deriv, grad_finalize (the gradient's own, veto rule included).
// The entries of v that are 0 columns of the gradient are never read; R's is not read either when the row has no taps (R <= velstep).

namespace {

struct RowTangent { double vR, vc; };

__device__ __forceinline__ RowTangent row_tangent(const GradArgs& a, int r, const RowInfo& ri) {
    const double* v = a.V + (size_t)r * a.ndim;
    RowTangent o;
    o.vR = (a.freespecres && (a.jax || ri.n > 0)) ? v[0] : 0.0;
    o.vc = a.freecont ? v[a.freespecres ? 1 : 0] : 0.0;
    return o;
}

}  // namespace

// d2 w_k / dR2 of the normalised taps: with c_k = k^2 - sum_j w_j j^2 and var = sum_j w_j c_j^2,
//     d2 w_k / dsigma2 = w_k ((c_k^2 - var) / sigma^6 - 3 c_k / sigma^4),   dsigma/dR constant.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_taps_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    const int r = blockIdx.x;
    const int t = threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const int n = ri.n;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    double* ddtaps = a.ddtaps + (size_t)r * a.tapcap;
    const double sigma = (ri.R / kFwhmToSigma) / a.velstep;
    double m2 = 0.0;
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        m2 += taps[k] * dk * dk;
    }
    m2 = block_sum(m2, lds);
    double var = 0.0;
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        const double c = dk * dk - m2;
        var += taps[k] * c * c;
    }
    var = block_sum(var, lds);
    const double s2 = sigma * sigma, is4 = 1.0 / (s2 * s2), is6 = is4 / s2;
    const double dsdR = 1.0 / (kFwhmToSigma * a.velstep);
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        const double c = dk * dk - m2;
        ddtaps[k] = (!a.jax && n == 0) ? 0.0 : taps[k] * ((c * c - var) * is6 - 3.0 * c * is4) * (dsdR * dsdR);
    }
}

// q, dq and the continuum / R partials of H v: ONE tap loop gives L(F), (dL/dR) F, (d2L/dR2) F, L(T), (dL/dR) T.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_model_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const RowTangent rt = row_tangent(a, r, ri);
    const double* F = a.F + (size_t)r * a.npix;
    const double* T = a.q + (size_t)r * a.npix;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    const double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    const double* ddtaps = a.ddtaps + (size_t)r * a.tapcap;
    double pc = 0.0, pR = 0.0;
    if (i < a.npix) {
        double cF, cT, rF = 0.0, rT = 0.0, rrF = 0.0;
        if (a.jax) {
            const int h = ri.n;
            if (i < h || i >= a.npix - h) {
                cF = F[i]; cT = T[i];                                              // edge reset
            } else {
                double c = 0.0, d = 0.0, dd = 0.0, ct = 0.0, dt = 0.0;
                for (int k = 0; k <= 2 * h; ++k) {
                    const double f = F[i + k - h], tt = T[i + k - h];
                    c += taps[k] * f;
                    d += dtaps[k] * f;
                    dd += ddtaps[k] * f;
                    ct += taps[k] * tt;
                    dt += dtaps[k] * tt;
                }
                cF = c; rF = d; rrF = dd; cT = ct; rT = dt;
            }
        } else if (ri.n > 0) {
            const int n = ri.n;
            int j = (int)(((long)i - n) % a.npix);
            if (j < 0) j += a.npix;
            double c = 0.0, d = 0.0, dd = 0.0, ct = 0.0, dt = 0.0;
            for (int k = 0; k <= 2 * n; ++k) {                                     // periodic boundary
                const double f = F[j], tt = T[j];
                c += taps[k] * f;
                d += dtaps[k] * f;
                dd += ddtaps[k] * f;
                ct += taps[k] * tt;
                dt += dtaps[k] * tt;
                if (++j == a.npix) j = 0;
            }
            cF = c / ri.bot; rF = d / ri.bot; rrF = dd / ri.bot; cT = ct / ri.bot; rT = dt / ri.bot;
        } else {
            cF = F[i]; cT = T[i];                                                  // R <= velstep: no convolution
        }
        const double is2 = a.ispec2[i];
        const double res = a.obj[i] - ri.cont * cF;
        const double term = is2 * res * res - a.lgis[i];
        const bool drop = isnan(term);                                             // the pixels nansum drops: W = 0
        const double dM = ri.cont * cT + rt.vc * cF + rt.vR * ri.cont * rF;
        const double qv = drop ? 0.0 : is2 * res;
        const double dqv = drop ? 0.0 : -is2 * dM;
        a.hq[(size_t)r * a.npix + i] = qv;
        a.hdq[(size_t)r * a.npix + i] = dqv;
        pc = dqv * cF + qv * (cT + rt.vR * rF);
        pR = (dqv * ri.cont + qv * rt.vc) * rF + qv * ri.cont * (rT + rt.vR * rrF);
    }
    pc = block_sum(pc, lds);
    pR = block_sum(pR, lds);
    if (threadIdx.x == 0) {
        double* out = a.part + ((size_t)r * a.ntiles + blockIdx.x) * a.ndim;
        if (a.freespecres) out[0] = (a.jax || ri.n > 0) ? pR : 0.0;
        if (a.freecont) out[a.freespecres ? 1 : 0] = pc;
        out[a.startind] = 0.0;                                                     // the ncomp slot
    }
}

// g and dg in place of F and T: ONE tap loop gives L^T q, (dL/dR)^T q, L^T dq.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_adjoint_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const RowTangent rt = row_tangent(a, r, ri);
    const double* q = a.hq + (size_t)r * a.npix;
    const double* dq = a.hdq + (size_t)r * a.npix;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    const double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    double lq, rq = 0.0, ldq;
    if (a.jax) {
        const int h = ri.n;
        const bool edge = i < h || i >= a.npix - h;
        lq = edge ? q[i] : 0.0;
        ldq = edge ? dq[i] : 0.0;
        // interior outputs o = i - k + h with tap k read pixel i
        const int klo = max(0, i + 2 * h - a.npix + 1), khi = min(2 * h, i);
        for (int k = klo; k <= khi; ++k) {
            const double qo = q[i - k + h];
            lq += taps[k] * qo;
            rq += dtaps[k] * qo;
            ldq += taps[k] * dq[i - k + h];
        }
    } else if (ri.n > 0) {
        const int n = ri.n;
        int j = (int)(((long)i + n) % a.npix);
        double c = 0.0, d = 0.0, cd = 0.0;
        for (int k = 0; k <= 2 * n; ++k) {                                         // output j read pixel i through tap k
            const double qo = q[j];
            c += taps[k] * qo;
            d += dtaps[k] * qo;
            cd += taps[k] * dq[j];
            if (--j < 0) j = a.npix - 1;
        }
        lq = c / ri.bot; rq = d / ri.bot; ldq = cd / ri.bot;
    } else {
        lq = q[i]; ldq = dq[i];
    }
    double* F = a.F + (size_t)r * a.npix;
    double* T = a.q + (size_t)r * a.npix;
    const double f = F[i], tt = T[i];
    F[i] = -f * ri.cont * lq;
    T[i] = -(tt * ri.cont + f * rt.vc) * lq - f * ri.cont * (rt.vR * rq + ldq);
}

// The second-order Voigt pass: per active component the three sums of dg dtau/dtheta_k + g (d2tau/dtheta_k dtheta_k') v_k'.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_deriv_kernel(const GradArgs a) {
    __shared__ double lds[3 * kGradBlock];
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const bool valid = i < a.npix;
    const double g = valid ? a.F[(size_t)r * a.npix + i] : 0.0;
    const double dg = valid ? a.q[(size_t)r * a.npix + i] : 0.0;
    const double nu = valid ? a.nu[i] : a.nu[0];
    const double* v = a.V + (size_t)r * a.ndim;
    double* out = a.part + ((size_t)r * a.ntiles + blockIdx.x) * a.ndim;
    const int ncomp = ri.nc + a.nfill;                 // active targets, then the fillers
    for (int c = 0; c < ncomp; ++c) {
        const bool fill = c >= ri.nc;
        const int slot0 = fill ? a.ncompmax * a.nlines + (c - ri.nc) : c * a.nlines;
        const int nl = fill ? 1 : a.nlines;
        const int col = fill ? a.endind + 3 * (c - ri.nc) : 1 + 3 * c + a.startind;
        double tN = 0.0, tz = 0.0, tb = 0.0, tzz = 0.0, tzb = 0.0, tbb = 0.0;
        for (int l = 0; l < nl; ++l) {
            const double* rec = rec_of(a, r, slot0 + l);
            const double u = nu * rec[0] - rec[1], y = rec[2], K = rec[3], s = nu * rec[4], ib = rec[5];
            double wr, dr, e, d2, e2, e3;
            faddeeva_d2w(u, y, wr, dr, e, d2, e2, e3);
            tN += K * wr;                                   // tau
            tz += K * dr * s;                               // K H_u du/dz
            tb -= K * ib * e;                               // -(K/b) Re (z w)'
            tzz += K * s * s * d2;
            tzb -= K * s * ib * e2;
            tbb += K * ib * ib * e3;
        }
        const double vN = kLn10 * v[col], vz = v[col + 1], vb = v[col + 2];
        double sN = kLn10 * (dg * tN + g * (tN * vN + tz * vz + tb * vb));
        double sz = dg * tz + g * (tz * vN + tzz * vz + tzb * vb);
        double sb = dg * tb + g * (tb * vN + tzb * vz + tbb * vb);
        block_sum3(sN, sz, sb, lds);
        if (threadIdx.x == 0) { out[col] = sN; out[col + 1] = sz; out[col + 2] = sb; }
    }
    if (threadIdx.x == 0)
        for (int c = ri.nc; c < a.ncompmax; ++c) {     // inactive components: exactly 0
            const int col = 1 + 3 * c + a.startind;
            out[col] = out[col + 1] = out[col + 2] = 0.0;
        }
}

__global__ void mcalf_grad_hjert_kernel(const double* x, const double* y, long n, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double wr, wi, dr, di, e;
    faddeeva_dw(x[i], y[i], wr, wi, dr, di, e);
    out[3 * i] = wr;
    out[3 * i + 1] = dr;          // dH/dx = Re w'
    out[3 * i + 2] = -di;         // dH/dy = Re(i w') = -Im w'
}

namespace mcalf {
const void* grad_setup_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_setup_kernel); }
const void* grad_forward_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_forward_kernel); }
const void* grad_model_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_model_kernel); }
const void* grad_adjoint_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_adjoint_kernel); }
const void* grad_deriv_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_deriv_kernel); }
const void* grad_finalize_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_finalize_kernel); }
const void* vjp_model_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_vjp_model_kernel); }
const void* vjp_finalize_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_vjp_finalize_kernel); }
const void* jvp_forward_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_jvp_forward_kernel); }
const void* jvp_model_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_jvp_model_kernel); }
const void* hvp_taps_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_hvp_taps_kernel); }
const void* hvp_model_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_hvp_model_kernel); }
const void* hvp_adjoint_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_hvp_adjoint_kernel); }
const void* hvp_deriv_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_hvp_deriv_kernel); }
const void* grad_hjert_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_grad_hjert_kernel); }
}  // namespace mcalf
